"""An independent float64 statement of the temporal stage of one rt_denoise_temporal call under rt_denoise_temporal_motion, in numpy
(float64 by default, float32 on request): where the history of a pixel on a moved triangle is looked up, which taps count, the
moments, the history length h and the integrated colour, with 0 iterations.

Written from DESIGN.md sections 10 and 15 and from Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017), not from the
project's sources: it imports nothing but numpy, opens no file and calls no project library, so a mistake in csrc/denoise_motion.h,
csrc/temporal_motion.h or csrc/denoise_math.h (which the kernel and tests/denoise_motion_ref.py share) is not shared by it. Every tap
is one whole-image gather, as in tests/denoise_spec.py, whose temporal stage this restates on the lookup point and normal (x_l, n_l).

Measured by tests/test_denoise_motion_spec_cpu.py (worst over its sequences at 40 x 33 and 64 x 48; error of the restatement /
spread / tol = 8 x spread, bar 1e-4):
  mu1     4.4e-6 / 4.4e-6 / 3.5e-5  (the box by (0.4, 0, 0.3) under the orbit, 40 x 33, call 3)
  mu2     1.0e-5 / 1.0e-5 / 8.1e-5  (the same call)
  colour  3.0e-6 / 3.0e-6 / 2.4e-5  (the same sequence at 64 x 48, call 2)
  left out for a decision margin below 1e-4: no pixel of any call (cap 2 %); h exact on all participating pixels.
"""
import numpy as np

REC709 = (0.2126, 0.7152, 0.0722)
ALPHA = dict(alpha_color=0.2, alpha_moments=0.2)  # SVGF section 4.1
TAP_NORMAL_MIN, TAP_PLANE_MAX, HISTORY_WEIGHT_MIN, HISTORY_MAX = 0.9, 2.0, 0.01, 32.0


def _quiet():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def _surface(v, bu, bv, eye, ft):
    """the point with barycentrics (u, v) on triangles v (.., 9) and the unit normal turned toward `eye`"""
    v0, v1, v2 = v[..., 0:3], v[..., 3:6], v[..., 6:9]
    x = (ft(1) - bu - bv) * v0 + bu * v1 + bv * v2
    n = _unit(np.cross(v1 - v0, v2 - v0))
    n = np.where((_dot(_unit(eye - x), n) < 0)[..., None], -n, n)
    return x, n


def temporal_stage(W, H, tris, vis, eye, rg, accum, prev, motion=None, dtype=np.float64, **params):
    """prev: the previous call's state, a dict of (W * H, 4) float32 arrays gx = {x, f}, gn = {n, guide word}, hcol, hmom = {mu1, mu2,
    h, 0}, and rg = its RayGenerator as 9 floats {origin, right, up}. motion: None (the camera only) or a dict: tris_prev (the
    triangles as they were when the previous call ran), lo, hi (the moved range) and eye_prev.

    Returns a dict of (W * H, ..) arrays: part, on_range, moments {mu1, mu2, h, 0}, colour (the integrated colour), margin (how far
    the float64 values are from the other outcome of a discrete decision: the seven of tests/denoise_spec.py, on the lookup point)."""
    ft = np.dtype(dtype).type
    p = dict(ALPHA)
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
    with _quiet():
        x, nrm = _surface(T, bu, bv, eye, ft)
        f = np.sqrt(_dot(x - eye, x - eye)) * (ft(2) * np.sqrt(_dot(rg9[6:9], rg9[6:9])) / ft(H))
        surface = hit & ~(T[:, 12:15] > 0).any(axis=-1)
        part = surface & (A[:, 3] != 0)
        albedo = T[:, 9:12]
        e = np.where(albedo > 0, (A[:, :3] / A[:, 3:4]) / albedo, ft(0))
    e = np.where(part[:, None], e, ft(0))
    lum = ft(REC709[0]) * e[:, 0] + ft(REC709[1]) * e[:, 1] + ft(REC709[2]) * e[:, 2]
    # a participating pixel on a triangle of the moved range looks up from where its point was
    xl, nl = x, nrm
    on_range = np.zeros(n_px, bool)
    if motion is not None:
        on_range = part & (index >= motion["lo"]) & (index < motion["hi"])
        tp = np.ascontiguousarray(motion["tris_prev"]).view(np.float32).reshape(-1, 15)[np.where(hit, index, 0)].astype(ft)
        with _quiet():
            xp, np_ = _surface(tp, bu, bv, np.asarray(motion["eye_prev"], np.float32).reshape(3).astype(ft), ft)
        xl, nl = np.where(on_range[:, None], xp, x), np.where(on_range[:, None], np_, nrm)
    pgx, pgn = (np.ascontiguousarray(prev[k], np.float32).reshape(n_px, 4) for k in ("gx", "gn"))
    hcol, hmom = (np.ascontiguousarray(prev[k], np.float32).reshape(n_px, 4).astype(ft) for k in ("hcol", "hmom"))
    psurface = (pgn[:, 3].copy().view(np.uint32) >> 30) == 0
    o, R, U = (np.asarray(prev["rg"], np.float32).reshape(9)[i:i + 3].astype(ft) for i in (0, 3, 6))
    F = _unit(np.cross(U, R))
    d = xl - o
    with _quiet():
        tt = _dot(d, F)
        a, b = _dot(d, R) / (tt * _dot(R, R)), _dot(d, U) / (tt * _dot(U, U))
        px, pr = (a + ft(1)) / ft(2) * ft(W), ft(H - 1) - (ft(1) - b) / ft(2) * ft(H)
        t_rel = tt / np.sqrt(_dot(d, d))
        in_range = part & (tt > 0) & (px >= -1) & (px < W) & (pr >= -1) & (pr < H)
        edge = np.minimum.reduce([np.abs(px + 1), np.abs(px - W), np.abs(pr + 1), np.abs(pr - H)]).astype(np.float64)
    inf = np.full(n_px, np.inf)
    m_behind = np.where(part & np.isfinite(t_rel), np.abs(t_rel).astype(np.float64), inf)
    m_range = np.where(part & (tt > 0) & np.isfinite(edge), edge, inf)
    pxs, prs = np.where(in_range, px, ft(0)), np.where(in_range, pr, ft(0))
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
        limit = (ft(TAP_PLANE_MAX) * f)[:, None]  # the current pixel's footprint
        valid = usable & (cosine >= ft(TAP_NORMAL_MIN)) & (offset <= limit)
        m_n = np.where(usable, np.abs(cosine - ft(TAP_NORMAL_MIN)) / ft(TAP_NORMAL_MIN), np.inf)
        m_p = np.where(usable, np.abs(offset - limit) / limit, np.inf)
        m_n, m_p = np.where(np.isnan(m_n), np.inf, m_n).min(axis=-1), np.where(np.isnan(m_p), np.inf, m_p).min(axis=-1)
    wv = np.where(valid, wts, ft(0))
    sw = wv.sum(axis=-1)
    m_w = np.where(usable.any(axis=-1), np.abs(sw - ft(HISTORY_WEIGHT_MIN)).astype(np.float64) / HISTORY_WEIGHT_MIN, inf)
    has = in_range & (sw >= ft(HISTORY_WEIGHT_MIN))
    first = np.argmax(wv, axis=-1)
    h_prev = np.take_along_axis(hq, first[:, None], axis=-1)[:, 0]
    w_first = np.take_along_axis(wv, first[:, None], axis=-1)[:, 0]
    other = np.where(valid & (hq != h_prev[:, None]), wts, ft(-np.inf)).max(axis=-1)
    m_h = np.where(has & np.isfinite(other), (w_first - other).astype(np.float64), inf)
    with _quiet():
        c_prev = (wv[..., None] * hcol[qi][..., :3]).sum(axis=-2) / sw[:, None]
        m1_prev, m2_prev = (wv * hmom[qi, 0]).sum(axis=-1) / sw, (wv * hmom[qi, 1]).sum(axis=-1) / sw
        h_new = np.minimum(h_prev + ft(1), ft(HISTORY_MAX))
        a_c, a_m = np.maximum(ft(p["alpha_color"]), ft(1) / h_new), np.maximum(ft(p["alpha_moments"]), ft(1) / h_new)
        col = np.where(has[:, None], (ft(1) - a_c)[:, None] * c_prev + a_c[:, None] * e, e)
        mu1 = np.where(has, (ft(1) - a_m) * m1_prev + a_m * lum, lum)
        mu2 = np.where(has, (ft(1) - a_m) * m2_prev + a_m * (lum * lum), lum * lum)
    z = ft(0)
    moments = np.zeros((n_px, 4), ft)
    moments[:, 0], moments[:, 1] = np.where(part, mu1, z), np.where(part, mu2, z)
    moments[:, 2] = np.where(part, np.where(has, h_new, ft(1)), z)
    margin = np.where(part, np.minimum.reduce([m_behind, m_range, m_n.astype(np.float64), m_p.astype(np.float64), m_w, m_h]), np.inf)
    return dict(part=part, on_range=on_range, moments=moments, colour=np.where(part[:, None], col, z), margin=margin,
                lookup=np.where(part[:, None], xl, z))
