"""An independent reference of rt_denoise and of one rt_denoise_temporal call, in numpy (float64 by default, float32 on request).

Written from the papers and from DESIGN.md sections 9 and 10, not from the project's sources: it imports nothing but numpy, opens
no file and calls no project library, so a mistake in csrc/denoise_math.h (which the kernels and the C++ restatements
tests/denoise_ref.py and tests/denoise_temporal_ref.py share) is not shared by it. It also has another shape than the kernels:
every tap is one whole-image operation on a shifted (or, for the reprojection, gathered) copy of the image, so there is no
per-pixel tap loop whose order or bounds could be copied.

Sources of the constants:
  [D10] Dammertz, Sewtz, Hanika, Lensch, "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010
  [S17] Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017
  [DES] DESIGN.md sections 9 ("Arithmetic") and 10 ("Arithmetic")

Inputs are those of the restatements: the image size, the scene's triangles (15 floats each: three vertices, albedo, emission),
the guide's rt_visibility records {u, v, triangle, pad} in storage order, the eye, the RayGenerator {origin, right, up}, the
accumulation buffer {rgb sum, w} and the parameters; the temporal call also takes the previous call's state.
"""
import numpy as np

# [D10] section 2: the B3-spline h = (1/16, 1/4, 3/8, 1/4, 1/16), applied separably as a 5 x 5 kernel with holes
B3 = {-2: 1.0 / 16.0, -1: 1.0 / 4.0, 0: 3.0 / 8.0, 1: 1.0 / 4.0, 2: 1.0 / 16.0}
# [S17] section 4.4: the variance is prefiltered with a 3 x 3 Gaussian, (1/4, 1/2, 1/4) separably
G3 = {-1: 1.0 / 4.0, 0: 1.0 / 2.0, 1: 1.0 / 4.0}
# ITU-R BT.709 luminance of linear RGB, the luminance of [S17]'s implementation
REC709 = (0.2126, 0.7152, 0.0722)
# [DES] section 9: both edge-stopping distances have this added to their denominator
EPS = 1e-10
# [S17] section 4.4 (sigma_l = 4, sigma_n = 128, sigma_z = 1), section 4.2 (7 x 7 window); [DES] section 9: 5 levels
SPATIAL_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=1.0, normal_power_log2=7, variance_radius=3)
# [S17] section 4.1: alpha = 0.2 for colour and moments
TEMPORAL_DEFAULTS = dict(alpha_color=0.2, alpha_moments=0.2)
# [DES] section 10: tap validity, history existence, history cap; [S17] section 4.2: the temporal variance from 4 frames on
TAP_NORMAL_MIN = 0.9
TAP_PLANE_MAX = 2.0
HISTORY_WEIGHT_MIN = 0.01
HISTORY_MAX = 32.0
HISTORY_VARIANCE_MIN = 4.0


def _quiet():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _rg9(rg):
    rg = np.asarray(rg)
    if rg.dtype.names:
        return np.concatenate([np.asarray(rg[k], np.float32).reshape(3) for k in ("origin", "right", "up")])
    return np.asarray(rg, np.float32).reshape(9)


class Guide:
    """Per pixel, as (H, W, ...) arrays in storage order: hit point x, normal n toward the eye, pixel footprint f, albedo, and
    the class: surface (a hit on a non-emissive triangle), emissive, or sky (no hit). [DES] section 9."""

    def __init__(self, W, H, tris, vis, eye, rg, ft):
        t = np.ascontiguousarray(tris).view(np.float32).reshape(-1, 15)
        v = np.ascontiguousarray(vis).view(np.float32).reshape(H, W, 4)
        index = v[..., 2].view(np.int32)
        hit = index >= 0
        T = t[np.where(hit, index, 0)].astype(ft)
        v0, v1, v2 = T[..., 0:3], T[..., 3:6], T[..., 6:9]
        bu, bv = v[..., 0:1].astype(ft), v[..., 1:2].astype(ft)
        eye = np.asarray(eye, np.float32).reshape(3).astype(ft)
        up = _rg9(rg)[6:9].astype(ft)
        with _quiet():
            x = (ft(1) - bu - bv) * v0 + bu * v1 + bv * v2
            n = _unit(np.cross(v1 - v0, v2 - v0))
            n = np.where((_dot(_unit(eye - x), n) < 0)[..., None], -n, n)
            # the image plane is 2 |up| tall at distance 1, so one of H pixel rows is 2 |up| / H wide there
            f = np.sqrt(_dot(x - eye, x - eye)) * (ft(2) * np.sqrt(_dot(up, up)) / ft(H))
        self.W, self.H, self.ft = W, H, ft
        self.hit = hit
        self.emissive = hit & (T[..., 12:15] > 0).any(axis=-1)
        self.surface = hit & ~self.emissive
        z = ft(0)
        self.x = np.where(hit[..., None], x, z)
        self.n = np.where(hit[..., None], n, z)
        self.f = np.where(hit, f, z)
        self.albedo = np.where(hit[..., None], T[..., 9:12], z)


def _shift(a, dy, dx, fill=0):
    """b[r, c] = a[r + dy, c + dx] where that is inside the image, `fill` elsewhere"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return b
    b[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = a[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return b


class _Coverage:
    """share of the off-centre taps between two participating pixels whose term lies in (0.05, 0.95), per edge-stopping term"""

    def __init__(self):
        self.n = dict(normal=[0, 0], plane=[0, 0], luminance=[0, 0])

    def add(self, term, value, taps):
        self.n[term][0] += int(((value > 0.05) & (value < 0.95) & taps).sum())
        self.n[term][1] += int(taps.sum())

    def shares(self):
        return {k: (a / b if b else 0.0) for k, (a, b) in self.n.items()}


def _geometry_terms(g, part, dy, dx, step, p, cov):
    """for the tap at offset (dy, dx) pixels: does it exist, the normal weight and the plane distance. [S17] eq. 3 and 4 in the
    form of [DES] section 9: w_n = max(0, n_p . n_q)^(2^k); D_x = |n_p . (x_q - x_p)| / (sigma_x * step * f_p + eps)"""
    ft = g.ft
    tap = part & _shift(part, dy, dx, False)
    nq, xq = _shift(g.n, dy, dx), _shift(g.x, dy, dx)
    with _quiet():
        wn = np.power(np.maximum(_dot(g.n, nq), ft(0)), ft(2 ** p["normal_power_log2"]))
        dist = np.abs(_dot(g.n, xq - g.x)) / (ft(p["sigma_plane"]) * ft(step) * g.f + ft(EPS))
    if cov is not None and (dy or dx):
        cov.add("normal", wn, tap)
        cov.add("plane", np.exp(-dist), tap)
    return tap, wn, dist


def _luminance(e, ft):
    return ft(REC709[0]) * e[..., 0] + ft(REC709[1]) * e[..., 1] + ft(REC709[2]) * e[..., 2]


def _window_variance(g, part, e, p, cov):
    """[S17] section 4.2's spatial estimate: max(0, E[l^2] - E[l]^2) over the (2R + 1)^2 window with the weights
    w_n * exp(-D_x) at step 1 ([DES] section 9: no luminance term here)"""
    ft, R = g.ft, p["variance_radius"]
    lum = _luminance(e, ft)
    sw, s1, s2 = (np.zeros(part.shape, ft) for _ in range(3))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            tap, wn, dist = _geometry_terms(g, part, dy, dx, 1, p, cov)
            with _quiet():
                w = np.where(tap, wn * np.exp(-dist), ft(0))
            lq = _shift(lum, dy, dx)
            sw += w
            s1 += w * lq
            s2 += w * (lq * lq)
    with _quiet():
        m1, m2 = s1 / sw, s2 / sw
        return np.where(part, np.maximum(m2 - m1 * m1, ft(0)), ft(0))


def _level(g, part, e, var, step, p, cov):
    """one a-trous level at hole size `step` ([D10] section 2, [S17] section 4.4): the variance prefiltered over the 3 x 3
    neighbourhood at the level's step, the weight h * w_n * exp(-(D_l + D_x)) with D_l = |l_p - l_q| / (sigma_l sqrt(g_p) + eps),
    e' = sum w e_q / sum w and var' = sum w^2 var_q / (sum w)^2"""
    ft = g.ft
    sk, sv = np.zeros(part.shape, ft), np.zeros(part.shape, ft)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            tap = part & _shift(part, dy * step, dx * step, False)
            k = ft(G3[dy] * G3[dx])
            sk += np.where(tap, k, ft(0))
            sv += np.where(tap, k * _shift(var, dy * step, dx * step), ft(0))
    lum = _luminance(e, ft)
    with _quiet():
        sd = ft(p["sigma_luminance"]) * np.sqrt(sv / sk) + ft(EPS)
    sw, svar, se = np.zeros(part.shape, ft), np.zeros(part.shape, ft), np.zeros(part.shape + (3,), ft)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            tap, wn, dist = _geometry_terms(g, part, oy, ox, step, p, cov)
            with _quiet():
                dl = np.abs(lum - _shift(lum, oy, ox)) / sd
                w = np.where(tap, ft(B3[dy] * B3[dx]) * wn * np.exp(-(dl + dist)), ft(0))
                if cov is not None and (dy or dx):
                    cov.add("luminance", np.exp(-dl), tap)
            sw += w
            se += w[..., None] * _shift(e, oy, ox)
            svar += (w * w) * _shift(var, oy, ox)
    with _quiet():
        e1 = np.where(part[..., None], se / sw[..., None], ft(0))
        var1 = np.where(part, svar / (sw * sw), ft(0))
    return e1, var1


def _demodulate(g, A, part):
    """[S17] section 4: e = (A.rgb / A.w) / albedo per channel, 0 where the albedo channel is 0 ([DES] section 9)"""
    ft = g.ft
    with _quiet():
        c = A[..., :3] / A[..., 3:4]
        e = np.where(g.albedo > 0, c / g.albedo, ft(0))
    return np.where(part[..., None], e, ft(0))


def _remodulate(g, A, part, e):
    """participating pixels: {e * albedo, 1}; the others keep their accumulation record"""
    out = np.empty(A.shape, g.ft)
    out[..., :3] = e * g.albedo
    out[..., 3] = 1
    return np.where(part[..., None], out, A)


def _record(part, e, var, ft):
    """the colour record {e, var} of a level; {0, 0, 0, -1} where the pixel does not participate"""
    r = np.zeros(part.shape + (4,), ft)
    r[..., :3] = e
    r[..., 3] = np.where(part, var, ft(-1))
    return r


def denoise(W, H, tris, vis, eye, rg, accum, dtype=np.float64, coverage=False, **params):
    """rt_denoise. Returns the HDR image (W * H, 4) and the participation mask (W * H); with coverage=True also the
    shares of taps whose normal, plane and luminance term lie in (0.05, 0.95)."""
    ft = np.dtype(dtype).type
    p = dict(SPATIAL_DEFAULTS)
    p.update(params)
    g = Guide(W, H, tris, vis, eye, rg, ft)
    A = np.ascontiguousarray(accum, np.float32).reshape(H, W, 4).astype(ft)
    part = g.surface & (A[..., 3] != 0)
    cov = _Coverage() if coverage else None
    e = _demodulate(g, A, part)
    var = _window_variance(g, part, e, p, cov)
    for i in range(p["iterations"]):
        e, var = _level(g, part, e, var, 1 << i, p, cov)
    out = _remodulate(g, A, part, e).reshape(-1, 4), part.reshape(-1)
    return out + (cov.shares(),) if coverage else out


def _reproject(g, prev_rg, W, H):
    """[DES] section 10: the hit point in the previous RayGenerator {o, R, U}, F = normalize(U x R): t = (x - o) . F,
    a = (x - o) . R / (t |R|^2), b = (x - o) . U / (t |U|^2), px = (a + 1) / 2 * W, pr = H - 1 - (1 - b) / 2 * H"""
    ft = g.ft
    o, R, U = (prev_rg[i:i + 3].astype(ft) for i in (0, 3, 6))
    F = _unit(np.cross(U, R))
    d = g.x - o
    with _quiet():
        t = _dot(d, F)
        a, b = _dot(d, R) / (t * _dot(R, R)), _dot(d, U) / (t * _dot(U, U))
        px = (a + ft(1)) / ft(2) * ft(W)
        pr = ft(H - 1) - (ft(1) - b) / ft(2) * ft(H)
        t_rel = t / np.sqrt(_dot(d, d))
    return t, t_rel, px, pr


def denoise_temporal(W, H, tris, vis, eye, rg, accum, prev=None, dtype=np.float64, **params):
    """One rt_denoise_temporal call. prev = None (no history) or the previous call's state as a dict of (W * H, 4) float32 arrays
    gx = {x, f}, gn = {n, guide word}, hcol = colour history, hmom = moments {mu1, mu2, h, 0}, and rg = its RayGenerator.

    Returns a dict: hdr (W * H, 4), moments (W * H, 4) = {mu1, mu2, h, 0}, history (W * H, 4) = {e, var} of the first level (of
    the integration with 0 iterations; {0, 0, 0, -1} where the pixel does not participate), part (W * H), decided (how many usable
    taps of weight >= 0.05 the normal test alone rejects, the plane test alone rejects, and both accept), margin (W * H) and
    margins (one array per decision). A margin is how far this evaluation is from the other outcome of a discrete decision:
      inside      px and pr from the image's first and last column and row, where a tap enters or leaves the image (pixels)
      range       px, pr from -1, W and H, the reprojection's range test (pixels)
      behind      t / |x - o| from 0
      normal      |n_p . n_q - 0.9| / 0.9 over the taps
      plane       ||n_p . (x_q - x_p)| - 2 f_p| / (2 f_p) over the taps
      weight      |sum w - 0.01| / 0.01
      heaviest    the gap between the two heaviest valid taps' weights where their h differ
    `margin` is the smallest of all but `inside`, which is reported but not part of it: a tap that enters or leaves the image
    there does so with a bilinear weight equal to that margin, so the result is continuous across it (a static camera puts every
    pixel of the first row and column there)."""
    ft = np.dtype(dtype).type
    p = dict(SPATIAL_DEFAULTS)
    p.update(TEMPORAL_DEFAULTS)
    p.update(params)
    n = W * H
    g = Guide(W, H, tris, vis, eye, rg, ft)
    A = np.ascontiguousarray(accum, np.float32).reshape(H, W, 4).astype(ft)
    part = g.surface & (A[..., 3] != 0)
    e = _demodulate(g, A, part)
    lum = _luminance(e, ft)
    inf = np.full((H, W), np.inf)
    margins = dict(inside=inf.copy(), range=inf.copy(), behind=inf.copy(), normal=inf.copy(), plane=inf.copy(), weight=inf.copy(),
                   heaviest=inf.copy())
    has = np.zeros((H, W), bool)
    decided = dict(normal_alone=0, plane_alone=0, both_pass=0)
    col, mu1, mu2, h = e, lum, lum * lum, np.where(part, ft(1), ft(0))
    if prev is not None:
        pgx, pgn = (np.ascontiguousarray(prev[k], np.float32).reshape(n, 4) for k in ("gx", "gn"))
        hcol, hmom = (np.ascontiguousarray(prev[k], np.float32).reshape(n, 4).astype(ft) for k in ("hcol", "hmom"))
        pword = pgn[:, 3].copy().view(np.uint32)
        psurface = (pword >> 30) == 0
        px_n, px_x = pgn[:, :3].astype(ft), pgx[:, :3].astype(ft)
        t, t_rel, px, pr = _reproject(g, _rg9(prev["rg"]), W, H)
        with _quiet():
            in_range = part & (t > 0) & (px >= -1) & (px < W) & (pr >= -1) & (pr < H)
        margins["behind"] = np.where(part, np.abs(t_rel).astype(np.float64), np.inf)
        pxs, prs = np.where(in_range, px, ft(0)), np.where(in_range, pr, ft(0))
        fx0, fr0 = np.floor(pxs), np.floor(prs)
        fx, fr = pxs - fx0, prs - fr0
        x0, r0 = fx0.astype(np.int64), fr0.astype(np.int64)
        ahead = part & (t > 0)
        with _quiet():
            edge = np.minimum.reduce([np.abs(px + 1), np.abs(px - W), np.abs(pr + 1), np.abs(pr - H)]).astype(np.float64)
            border = np.minimum.reduce([np.abs(px), np.abs(px - (W - 1)), np.abs(pr), np.abs(pr - (H - 1))]).astype(np.float64)
        margins["range"] = np.where(ahead & np.isfinite(edge), edge, np.inf)
        margins["inside"] = np.where(in_range, border, np.inf)
        # the 2 x 2 taps in the order r0x0, r0x1, r1x0, r1x1, gathered from the previous call's arrays
        wts = np.stack([(ft(1) - fx) * (ft(1) - fr), fx * (ft(1) - fr), (ft(1) - fx) * fr, fx * fr], axis=-1)
        qx = np.stack([x0, x0 + 1, x0, x0 + 1], axis=-1)
        qr = np.stack([r0, r0, r0 + 1, r0 + 1], axis=-1)
        inside = in_range[..., None] & (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
        qi = np.clip(qr, 0, H - 1) * W + np.clip(qx, 0, W - 1)
        hq = hmom[qi, 2]
        usable = inside & psurface[qi] & (hq > 0)
        cosine = _dot(g.n[:, :, None, :], px_n[qi])
        offset = np.abs(_dot(g.n[:, :, None, :], px_x[qi] - g.x[:, :, None, :]))
        limit = (ft(TAP_PLANE_MAX) * g.f)[..., None]
        valid = usable & (cosine >= ft(TAP_NORMAL_MIN)) & (offset <= limit)
        with _quiet():
            m_n = np.where(usable, np.abs(cosine - ft(TAP_NORMAL_MIN)) / ft(TAP_NORMAL_MIN), np.inf).min(axis=-1)
            m_p = np.where(usable, np.abs(offset - limit) / limit, np.inf).min(axis=-1)
        margins["normal"], margins["plane"] = m_n.astype(np.float64), m_p.astype(np.float64)
        # input coverage: usable taps of some weight that one of the two geometric tests alone rejects
        heavy, n_ok, p_ok = usable & (wts >= ft(0.05)), cosine >= ft(TAP_NORMAL_MIN), offset <= limit
        decided = dict(normal_alone=int((heavy & ~n_ok & p_ok).sum()), plane_alone=int((heavy & n_ok & ~p_ok).sum()),
                       both_pass=int((heavy & n_ok & p_ok).sum()))
        wv = np.where(valid, wts, ft(0))
        sw = wv.sum(axis=-1)
        any_usable = usable.any(axis=-1)
        margins["weight"] = np.where(any_usable, np.abs(sw - ft(HISTORY_WEIGHT_MIN)).astype(np.float64) / HISTORY_WEIGHT_MIN, np.inf)
        has = in_range & (sw >= ft(HISTORY_WEIGHT_MIN))
        # h of the heaviest valid tap (the first on ties); the margin is the gap to the next tap with another h
        first = np.argmax(wv, axis=-1)
        h_prev = np.take_along_axis(hq, first[..., None], axis=-1)[..., 0]
        w_first = np.take_along_axis(wv, first[..., None], axis=-1)[..., 0]
        other = np.where(valid & (hq != h_prev[..., None]), wts, ft(-np.inf)).max(axis=-1)
        margins["heaviest"] = np.where(has & np.isfinite(other), (w_first - other).astype(np.float64), np.inf)
        with _quiet():
            c_prev = (wv[..., None] * hcol[qi][..., :3]).sum(axis=-2) / sw[..., None]
            m1_prev = (wv * hmom[qi, 0]).sum(axis=-1) / sw
            m2_prev = (wv * hmom[qi, 1]).sum(axis=-1) / sw
            # [S17] section 4.1 with the history cap of [DES] section 10: h = min(h' + 1, 32), alpha = max(alpha, 1 / h)
            h_new = np.minimum(h_prev + ft(1), ft(HISTORY_MAX))
            a_c = np.maximum(ft(p["alpha_color"]), ft(1) / h_new)
            a_m = np.maximum(ft(p["alpha_moments"]), ft(1) / h_new)
            col = np.where(has[..., None], (ft(1) - a_c)[..., None] * c_prev + a_c[..., None] * e, e)
            mu1 = np.where(has, (ft(1) - a_m) * m1_prev + a_m * lum, lum)
            mu2 = np.where(has, (ft(1) - a_m) * m2_prev + a_m * (lum * lum), lum * lum)
        h = np.where(part, np.where(has, h_new, ft(1)), ft(0))
    z = ft(0)
    col = np.where(part[..., None], col, z)
    mu1, mu2 = np.where(part, mu1, z), np.where(part, mu2, z)
    # [S17] section 4.2: the temporal variance where the history is long enough, the spatial window elsewhere
    var = np.where(h >= ft(HISTORY_VARIANCE_MIN), np.maximum(mu2 - mu1 * mu1, z), _window_variance(g, part, col, p, None))
    var = np.where(part, var, z)
    ecur, history = col, _record(part, col, var, ft)
    for i in range(p["iterations"]):
        ecur, var = _level(g, part, ecur, var, 1 << i, p, None)
        if i == 0:
            history = _record(part, ecur, var, ft)
    moments = np.zeros((H, W, 4), ft)
    moments[..., 0], moments[..., 1], moments[..., 2] = mu1, mu2, h
    margin = np.minimum.reduce([margins[k] for k in ("behind", "range", "normal", "plane", "weight", "heaviest")])
    margin = np.where(part, margin, np.inf)
    return dict(hdr=_remodulate(g, A, part, ecur).reshape(-1, 4), moments=moments.reshape(-1, 4), history=history.reshape(-1, 4),
                part=part.reshape(-1), margin=margin.reshape(-1), decided=decided, margins={k: v.reshape(-1) for k, v in margins.items()})
