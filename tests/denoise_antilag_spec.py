"""An independent float64 statement of one rt_denoise_temporal call under rt_denoise_temporal_antilag (and, where the caller passes
`motion`, under rt_denoise_temporal_motion as well), in numpy (float64 by default, float32 on request): the lookup, the taps, the
window gradient and lambda', the adapted blend of colour and moments, the variance, the a-trous levels and the image.

Written from DESIGN.md sections 9, 10, 15 and 19, from Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017) and
Dammertz et al., "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering" (HPG 2010), not from the project's
sources: it imports nothing but numpy, opens no file and calls no project library, so a mistake in csrc/denoise_antilag.h or the
other headers (which the kernels and tests/denoise_antilag_ref.py share) is not shared by it. It has another shape than the kernels:
every tap and every window offset is one whole-image operation on a shifted or gathered copy, and the window sums are formed for
every pixel whether or not it will use them.

Measured by tests/test_denoise_antilag_spec_cpu.py (worst over its sequences; error of the restatement / spread / tol = 8 x spread,
bar 1e-4): see MEASURED in that file.
"""
import numpy as np

B3 = {-2: 1.0 / 16.0, -1: 1.0 / 4.0, 0: 3.0 / 8.0, 1: 1.0 / 4.0, 2: 1.0 / 16.0}  # Dammertz et al., section 2
G3 = {-1: 1.0 / 4.0, 0: 1.0 / 2.0, 1: 1.0 / 4.0}                                 # Schied et al., section 4.4
REC709 = (0.2126, 0.7152, 0.0722)
EPS = 1e-10
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=1.0, normal_power_log2=7, variance_radius=3, alpha_color=0.2, alpha_moments=0.2)
TAP_NORMAL_MIN, TAP_PLANE_MAX, HISTORY_WEIGHT_MIN, HISTORY_MAX, HISTORY_VARIANCE_MIN = 0.9, 2.0, 0.01, 32.0, 4.0
WINDOW_NORMAL_MIN = 0.9  # a member of the window needs n_p . n_q >= this


def _quiet():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _lum(e, ft):
    return ft(REC709[0]) * e[..., 0] + ft(REC709[1]) * e[..., 1] + ft(REC709[2]) * e[..., 2]


def _shift(a, dy, dx, fill=0):
    """b[r, c] = a[r + dy, c + dx] where that is inside the image, `fill` elsewhere"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return b
    b[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = a[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return b


def _surface(T, bu, bv, eye, ft):
    v0, v1, v2 = T[..., 0:3], T[..., 3:6], T[..., 6:9]
    x = (ft(1) - bu - bv) * v0 + bu * v1 + bv * v2
    n = _unit(np.cross(v1 - v0, v2 - v0))
    return x, np.where((_dot(_unit(eye - x), n) < 0)[..., None], -n, n)


def _geometry(x, n, f, part, dy, dx, step, p, ft):
    tap = part & _shift(part, dy, dx, False)
    with _quiet():
        wn = np.power(np.maximum(_dot(n, _shift(n, dy, dx)), ft(0)), ft(2 ** p["normal_power_log2"]))
        dist = np.abs(_dot(n, _shift(x, dy, dx) - x)) / (ft(p["sigma_plane"]) * ft(step) * f + ft(EPS))
    return tap, wn, dist


def _window_variance(x, n, f, part, e, p, ft):
    R = p["variance_radius"]
    lum = _lum(e, ft)
    sw, s1, s2 = (np.zeros(part.shape, ft) for _ in range(3))
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            tap, wn, dist = _geometry(x, n, f, part, dy, dx, 1, p, ft)
            with _quiet():
                w = np.where(tap, wn * np.exp(-dist), ft(0))
            lq = _shift(lum, dy, dx)
            sw, s1, s2 = sw + w, s1 + w * lq, s2 + w * (lq * lq)
    with _quiet():
        m1, m2 = s1 / sw, s2 / sw
        return np.where(part, np.maximum(m2 - m1 * m1, ft(0)), ft(0))


def _level(x, n, f, part, e, var, step, p, ft):
    sk, sv = np.zeros(part.shape, ft), np.zeros(part.shape, ft)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            tap = part & _shift(part, dy * step, dx * step, False)
            k = ft(G3[dy] * G3[dx])
            sk, sv = sk + np.where(tap, k, ft(0)), sv + np.where(tap, k * _shift(var, dy * step, dx * step), ft(0))
    lum = _lum(e, ft)
    with _quiet():
        sd = ft(p["sigma_luminance"]) * np.sqrt(sv / sk) + ft(EPS)
    sw, svar, se = np.zeros(part.shape, ft), np.zeros(part.shape, ft), np.zeros(part.shape + (3,), ft)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            tap, wn, dist = _geometry(x, n, f, part, oy, ox, step, p, ft)
            with _quiet():
                dl = np.abs(lum - _shift(lum, oy, ox)) / sd
                w = np.where(tap, ft(B3[dy] * B3[dx]) * wn * np.exp(-(dl + dist)), ft(0))
            sw, se, svar = sw + w, se + w[..., None] * _shift(e, oy, ox), svar + (w * w) * _shift(var, oy, ox)
    with _quiet():
        return np.where(part[..., None], se / sw[..., None], ft(0)), np.where(part, svar / (sw * sw), ft(0))


def _record(part, e, var, ft):
    r = np.zeros(part.shape + (4,), ft)
    r[..., :3] = e
    r[..., 3] = np.where(part, var, ft(-1))
    return r


def call(W, H, tris, vis, eye, rg, accum, prev, antilag=None, motion=None, dtype=np.float64, **params):
    """One call with a history. prev: the previous call's state, a dict of (W * H, 4) float32 arrays gx = {x, f}, gn = {n, guide word},
    hcol, hmom = {mu1, mu2, h, .} and rg = its RayGenerator as 9 floats {origin, right, up}. antilag: None (the toggle off) or a dict
    radius, gradient_lo, gradient_hi, floor. motion: None (the camera only) or a dict tris_prev, lo, hi, eye_prev.

    Returns (W * H, ..) arrays: part, has (a history of its own), moments {mu1, mu2, h, lambda'}, colour (the integrated colour),
    history ({e, var} after the first level; the integration with 0 iterations), hdr, lam (the gradient, NaN where none is formed),
    members (the window's member count), margin (distance of this evaluation from the other outcome of a discrete decision of the
    lookup: behind, range, normal, plane, weight, heaviest tap) and member_margin (the same for the window's n_p . n_q >= 0.9, the
    smallest over the window's candidates: participating pixels with a history)."""
    ft = np.dtype(dtype).type
    p = dict(DEFAULTS)
    p.update(params)
    n_px = W * H
    t = np.ascontiguousarray(tris).view(np.float32).reshape(-1, 15)
    v = np.ascontiguousarray(vis).view(np.float32).reshape(n_px, 4)
    index = v[:, 2].copy().view(np.int32)
    hit = index >= 0
    T = t[np.where(hit, index, 0)].astype(ft)
    bu, bv = v[:, 0:1].astype(ft), v[:, 1:2].astype(ft)
    eye = np.asarray(eye, np.float32).reshape(3).astype(ft)
    rg9 = np.asarray(rg, np.float32).reshape(9).astype(ft)
    A = np.ascontiguousarray(accum, np.float32).reshape(n_px, 4).astype(ft)
    z = ft(0)
    with _quiet():
        x, nrm = _surface(T, bu, bv, eye, ft)
        f = np.sqrt(_dot(x - eye, x - eye)) * (ft(2) * np.sqrt(_dot(rg9[6:9], rg9[6:9])) / ft(H))
        albedo = T[:, 9:12]
        part = hit & ~(T[:, 12:15] > 0).any(axis=-1) & (A[:, 3] != 0)
        e = np.where(part[:, None], np.where(albedo > 0, (A[:, :3] / A[:, 3:4]) / albedo, z), z)
    x, nrm, f = np.where(hit[:, None], x, z), np.where(hit[:, None], nrm, z), np.where(hit, f, z)
    lum = _lum(e, ft)
    # section 15: a participating pixel on a triangle of the moved range looks up from where its point was
    xl, nl = x, nrm
    if motion is not None:
        on_range = part & (index >= motion["lo"]) & (index < motion["hi"])
        tp = np.ascontiguousarray(motion["tris_prev"]).view(np.float32).reshape(-1, 15)[np.where(hit, index, 0)].astype(ft)
        with _quiet():
            xp, np_ = _surface(tp, bu, bv, np.asarray(motion["eye_prev"], np.float32).reshape(3).astype(ft), ft)
        xl, nl = np.where(on_range[:, None], xp, x), np.where(on_range[:, None], np_, nrm)
    # section 10: reprojection into the previous RayGenerator, 2 x 2 taps
    pgx, pgn = (np.ascontiguousarray(prev[k], np.float32).reshape(n_px, 4) for k in ("gx", "gn"))
    hcol, hmom = (np.ascontiguousarray(prev[k], np.float32).reshape(n_px, 4).astype(ft) for k in ("hcol", "hmom"))
    psurface = (pgn[:, 3].copy().view(np.uint32) >> 30) == 0
    o, Rr, U = (np.asarray(prev["rg"], np.float32).reshape(9)[i:i + 3].astype(ft) for i in (0, 3, 6))
    F = _unit(np.cross(U, Rr))
    d = xl - o
    inf = np.full(n_px, np.inf)
    with _quiet():
        tt = _dot(d, F)
        a, b = _dot(d, Rr) / (tt * _dot(Rr, Rr)), _dot(d, U) / (tt * _dot(U, U))
        px, pr = (a + ft(1)) / ft(2) * ft(W), ft(H - 1) - (ft(1) - b) / ft(2) * ft(H)
        t_rel = tt / np.sqrt(_dot(d, d))
        in_range = part & (tt > 0) & (px >= -1) & (px < W) & (pr >= -1) & (pr < H)
        edge = np.minimum.reduce([np.abs(px + 1), np.abs(px - W), np.abs(pr + 1), np.abs(pr - H)]).astype(np.float64)
    m_behind = np.where(part & np.isfinite(t_rel), np.abs(t_rel).astype(np.float64), inf)
    m_range = np.where(part & (tt > 0) & np.isfinite(edge), edge, inf)
    pxs, prs = np.where(in_range, px, z), np.where(in_range, pr, z)
    fx0, fr0 = np.floor(pxs), np.floor(prs)
    fx, fr = pxs - fx0, prs - fr0
    x0, r0 = fx0.astype(np.int64), fr0.astype(np.int64)
    wts = np.stack([(ft(1) - fx) * (ft(1) - fr), fx * (ft(1) - fr), (ft(1) - fx) * fr, fx * fr], axis=-1)
    qx, qr = np.stack([x0, x0 + 1, x0, x0 + 1], axis=-1), np.stack([r0, r0, r0 + 1, r0 + 1], axis=-1)
    inside = in_range[:, None] & (qx >= 0) & (qx < W) & (qr >= 0) & (qr < H)
    qi = np.clip(qr, 0, H - 1) * W + np.clip(qx, 0, W - 1)
    hq = hmom[qi, 2]
    usable = inside & psurface[qi] & (hq > 0)
    with _quiet():
        cosine = _dot(nl[:, None, :], pgn[qi][..., :3].astype(ft))
        offset = np.abs(_dot(nl[:, None, :], pgx[qi][..., :3].astype(ft) - xl[:, None, :]))
        limit = (ft(TAP_PLANE_MAX) * f)[:, None]
        valid = usable & (cosine >= ft(TAP_NORMAL_MIN)) & (offset <= limit)
        m_n = np.where(usable, np.abs(cosine - ft(TAP_NORMAL_MIN)) / ft(TAP_NORMAL_MIN), np.inf)
        m_p = np.where(usable, np.abs(offset - limit) / limit, np.inf)
        m_n, m_p = np.where(np.isnan(m_n), np.inf, m_n).min(axis=-1), np.where(np.isnan(m_p), np.inf, m_p).min(axis=-1)
    wv = np.where(valid, wts, z)
    sw = wv.sum(axis=-1)
    m_w = np.where(usable.any(axis=-1), np.abs(sw - ft(HISTORY_WEIGHT_MIN)).astype(np.float64) / HISTORY_WEIGHT_MIN, inf)
    has = in_range & (sw >= ft(HISTORY_WEIGHT_MIN))
    first = np.argmax(wv, axis=-1)
    h_prev = np.take_along_axis(hq, first[:, None], axis=-1)[:, 0]
    w_first = np.take_along_axis(wv, first[:, None], axis=-1)[:, 0]
    other = np.where(valid & (hq != h_prev[:, None]), wts, ft(-np.inf)).max(axis=-1)
    m_h = np.where(has & np.isfinite(other), (w_first - other).astype(np.float64), inf)
    margin = np.where(part, np.minimum.reduce([m_behind, m_range, m_n.astype(np.float64), m_p.astype(np.float64), m_w, m_h]), np.inf)
    with _quiet():
        c_prev = (wv[..., None] * hcol[qi][..., :3]).sum(axis=-2) / sw[:, None]
        m1_prev, m2_prev = (wv * hmom[qi, 0]).sum(axis=-1) / sw, (wv * hmom[qi, 1]).sum(axis=-1) / sw
    c_prev = np.where(has[:, None], c_prev, z)
    # section 19: the gradient of window sums, current frame against reprojected history, over the members
    lam = np.full(n_px, np.nan)
    members = np.zeros(n_px, np.int64)
    member_margin = np.full(n_px, np.inf)
    lr = np.zeros(n_px, ft)
    if antilag is not None:
        R = int(antilag["radius"])
        img = lambda q: q.reshape((H, W) + q.shape[1:])  # noqa: E731
        n2, has2, le2, lh2 = img(nrm), img(has), img(lum), img(_lum(c_prev, ft))
        mc, mh, cnt, mm = np.zeros((H, W), ft), np.zeros((H, W), ft), np.zeros((H, W), np.int64), np.full((H, W), np.inf)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                cand = _shift(has2, dy, dx, False)
                cos_w = _dot(n2, _shift(n2, dy, dx))
                member = cand & (cos_w >= ft(WINDOW_NORMAL_MIN))
                mc, mh, cnt = mc + np.where(member, _shift(le2, dy, dx), z), mh + np.where(member, _shift(lh2, dy, dx), z), cnt + member
                mm = np.minimum(mm, np.where(cand, np.abs(cos_w - ft(WINDOW_NORMAL_MIN)).astype(np.float64) / WINDOW_NORMAL_MIN, np.inf))
        with _quiet():
            den = np.maximum(mc, mh) + ft(antilag["floor"]) * cnt.astype(ft)
            lam2 = np.where(den > 0, np.abs(mc - mh) / den, z)
            lr2 = np.clip((lam2 - ft(antilag["gradient_lo"])) / (ft(antilag["gradient_hi"]) - ft(antilag["gradient_lo"])), z, ft(1))
        lr = np.where(has, lr2.reshape(-1), z)
        lam = np.where(has, lam2.reshape(-1).astype(np.float64), np.nan)
        members = np.where(has, cnt.reshape(-1), 0)
        member_margin = np.where(has, mm.reshape(-1), np.inf)
    with _quiet():
        h_new = np.minimum(h_prev + ft(1), ft(HISTORY_MAX))
        a_c = np.maximum(ft(p["alpha_color"]) + (ft(1) - ft(p["alpha_color"])) * lr, ft(1) / h_new)
        a_m = np.maximum(ft(p["alpha_moments"]) + (ft(1) - ft(p["alpha_moments"])) * lr, ft(1) / h_new)
        col = np.where(has[:, None], (ft(1) - a_c)[:, None] * c_prev + a_c[:, None] * e, e)
        mu1 = np.where(has, (ft(1) - a_m) * m1_prev + a_m * lum, lum)
        mu2 = np.where(has, (ft(1) - a_m) * m2_prev + a_m * (lum * lum), lum * lum)
    col = np.where(part[:, None], col, z)
    moments = np.zeros((n_px, 4), ft)
    moments[:, 0], moments[:, 1] = np.where(part, mu1, z), np.where(part, mu2, z)
    moments[:, 2] = np.where(part, np.where(has, h_new, ft(1)), z)
    moments[:, 3] = np.where(part, lr, z)
    # sections 9 and 10: the variance (temporal from 4 frames on), the levels, the image
    sh = (H, W)
    X, N, Fp, P2 = x.reshape(sh + (3,)), nrm.reshape(sh + (3,)), f.reshape(sh), part.reshape(sh)
    ecur = col.reshape(sh + (3,))
    M1, M2, Hn = (moments[:, k].reshape(sh) for k in (0, 1, 2))
    var = np.where(Hn >= ft(HISTORY_VARIANCE_MIN), np.maximum(M2 - M1 * M1, z), _window_variance(X, N, Fp, P2, ecur, p, ft))
    var = np.where(P2, var, z)
    history = _record(P2, ecur, var, ft)
    for i in range(p["iterations"]):
        ecur, var = _level(X, N, Fp, P2, ecur, var, 1 << i, p, ft)
        if i == 0:
            history = _record(P2, ecur, var, ft)
    hdr = np.empty((n_px, 4), ft)
    hdr[:, :3], hdr[:, 3] = ecur.reshape(-1, 3) * albedo, 1
    hdr = np.where(part[:, None], hdr, A)
    return dict(part=part, has=has, moments=moments, colour=col, history=history.reshape(-1, 4), hdr=hdr, lam=lam, members=members,
                margin=margin, member_margin=member_margin)
