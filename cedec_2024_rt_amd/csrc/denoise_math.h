/*
 * denoise_math.h — per-pixel and per-tap arithmetic of rt_denoise (include/restir_rt_internal.h): a spatial edge-avoiding
 * a-trous wavelet filter (Dammertz et al. 2010, "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination
 * Filtering") with the variance-guided luminance weight of SVGF (Schied et al. 2017); and the temporal half of SVGF that
 * rt_denoise_temporal adds in front of it (reprojection into the previous camera, colour and moment history; the last section).
 *
 * Every formula the kernels (denoise_kernels.h) evaluate is here, as RT_HD functions over IEEE +, -, *, / and the two
 * portable transcendentals (pm_expf; sqrt_guarded, correctly rounded on both sides, rt_device.h). Compiled by hipcc and by
 * `g++ -ffp-contract=off` the same expressions give the same bits, so a CPU restatement of the loops
 * (tests/denoise_ref.py) equals the GPU bit for bit. The loops themselves (tap order: dy outer, dx inner) live in the
 * kernels and are restated by the test.
 *
 * Pixel classes (guide word = bits of the guide's second float4 .w): bits 31..30 = kind, bits 29..0 = triangle index.
 *   SURFACE  (kind 0): a hit on a non-emissive triangle; participates if its accumulation w != 0
 *   EMISSIVE (kind 1): a hit on an emissive triangle
 *   SKY      (kind 3): no hit (the word is the -1 of a miss)
 * Pixels that do not participate keep their accumulation value; they are never taps (their colour record has var = -1).
 *
 * Defaults (rt_denoise_params NULL): 5 iterations (steps 1, 2, 4, 8, 16), sigma_luminance 4, sigma_plane 1,
 * normal_power_log2 7 (n.n' ^ 128), variance_radius 3 (7 x 7). Not retuned; DESIGN.md section 9 has the measured quality (the
 * error goal met, the 3 % mean-luminance goal missed) and why a larger sigma_luminance does not close the gap.
 */
#pragma once
#include "rt_device.h"
#include "temporal_reproject.h"

namespace rt
{

#if !defined(__HIPCC__)
struct float4 /* the host restatement's stand-in for HIP's vector type (members only) */
{
    float x, y, z, w;
};
#endif

constexpr uint32_t DN_KIND_SURFACE = 0u, DN_KIND_EMISSIVE = 1u, DN_KIND_SKY = 3u;
RT_HD uint32_t dn_guide_word(int tri, bool emissive) { return tri < 0 ? 0xffffffffu : ((uint32_t)tri | (emissive ? DN_KIND_EMISSIVE << 30 : 0u)); }
RT_HD uint32_t dn_kind(uint32_t word) { return word >> 30; }
RT_HD int dn_tri(uint32_t word) { return (int)(word & 0x3fffffffu); }

/* 5-tap B3-spline of the a-trous levels and the 3-tap kernel of the variance prefilter */
RT_HD float dn_h1(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }
RT_HD float dn_k1(int d) { return d == 0 ? 0.5f : 0.25f; }

/* x_p, n_p: common/core.hpp:189-207 (frame_kernels.h surface_info) from the triangle's vertices, normal toward the eye */
RT_HD void dn_surface(f3 v0, f3 v1, f3 v2, float u, float v, f3 eye, f3& p, f3& n)
{
    p = (1.0f - u - v) * v0 + u * v1 + v * v2;
    n = tri_normal(v0, v1, v2);
    const f3 view = normalize(eye - p);
    if (dot(view, n) < 0.0f) n = -n;
}
/* f_p: world size of one pixel at the hit (the image plane of RayGenerator is 2 |up| tall at distance 1 along forward) */
RT_HD float dn_pixel_size(f3 p, f3 eye, f3 rg_up, int H) { return length(p - eye) * ((2.0f * length(rg_up)) / (float)H); }

/* demodulated irradiance e = (A.rgb / A.w) / albedo, per channel; 0 where the albedo channel is 0 */
RT_HD f3 dn_demodulate(float4 A, f3 a)
{
    const float cr = A.x / A.w, cg = A.y / A.w, cb = A.z / A.w;
    return F3(a.x > 0.0f ? cr / a.x : 0.0f, a.y > 0.0f ? cg / a.y : 0.0f, a.z > 0.0f ? cb / a.z : 0.0f);
}
RT_HD float dn_luminance(f3 e) { return 0.2126f * e.x + 0.7152f * e.y + 0.0722f * e.z; }
RT_HD float dn_luminance(float4 e) { return 0.2126f * e.x + 0.7152f * e.y + 0.0722f * e.z; }

/* max(0, n_p . n_q) squared `power_log2` times */
RT_HD float dn_normal_weight(f3 np, f3 nq, int power_log2)
{
    const float d = dot(np, nq);
    float w = d > 0.0f ? d : 0.0f;
    for (int i = 0; i < power_log2; ++i) w = w * w;
    return w;
}
/* D_x: distance of x_q from the tangent plane of p, in units of sigma_x * step pixels at p */
RT_HD float dn_plane_distance(f3 np, f3 xp, f3 xq, float sigma_x, float step, float fp)
{
    return fabsf(dot(np, xq - xp)) / (sigma_x * step * fp + 1e-10f);
}
/* D_l: luminance difference in units of sigma_l standard deviations (g = prefiltered variance at p) */
RT_HD float dn_luminance_distance(float lp, float lq, float sigma_l, float g) { return fabsf(lp - lq) / (sigma_l * sqrt_guarded(g) + 1e-10f); }
RT_HD float dn_tap_weight(float h, float wn, float dl, float dx) { return h * wn * pm_expf(-(dl + dx)); }
RT_HD float dn_variance_weight(float wn, float dx) { return wn * pm_expf(-dx); }

/* variance estimate over the window: sums in tap order, then max(0, E[l^2] - E[l]^2) */
struct DnMoments
{
    float sw, s1, s2;
};
RT_HD DnMoments dn_moments_init() { return DnMoments{0.0f, 0.0f, 0.0f}; }
RT_HD void dn_moments_add(DnMoments& m, float w, float l)
{
    m.sw = m.sw + w;
    m.s1 = m.s1 + w * l;
    m.s2 = m.s2 + w * (l * l);
}
RT_HD float dn_moments_variance(const DnMoments& m)
{
    const float m1 = m.s1 / m.sw, m2 = m.s2 / m.sw;
    const float v = m2 - m1 * m1;
    return v > 0.0f ? v : 0.0f;
}

/* the 3 x 3 prefilter of the variance: sums in tap order over the taps that exist and participate */
struct DnPrefilter
{
    float sk, sv;
};
RT_HD DnPrefilter dn_prefilter_init() { return DnPrefilter{0.0f, 0.0f}; }
RT_HD void dn_prefilter_add(DnPrefilter& g, float k, float var)
{
    g.sk = g.sk + k;
    g.sv = g.sv + k * var;
}
RT_HD float dn_prefilter_result(const DnPrefilter& g) { return g.sv / g.sk; }

/* one a-trous level: e' = sum w e_q / sum w, var' = sum w^2 var_q / (sum w)^2 */
struct DnFilter
{
    float sw, r, g, b, sv;
};
RT_HD DnFilter dn_filter_init() { return DnFilter{0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
RT_HD void dn_filter_add(DnFilter& f, float w, float4 eq)
{
    f.sw = f.sw + w;
    f.r = f.r + w * eq.x;
    f.g = f.g + w * eq.y;
    f.b = f.b + w * eq.z;
    f.sv = f.sv + (w * w) * eq.w;
}
RT_HD float4 dn_filter_result(const DnFilter& f)
{
    float4 o;
    o.x = f.r / f.sw;
    o.y = f.g / f.sw;
    o.z = f.b / f.sw;
    o.w = f.sv / (f.sw * f.sw);
    return o;
}
/* remodulated HDR value of a participating pixel */
RT_HD float4 dn_remodulate(float4 e, f3 a)
{
    float4 o;
    o.x = e.x * a.x;
    o.y = e.y * a.y;
    o.z = e.z * a.z;
    o.w = 1.0f;
    return o;
}

/* ---- temporal half (rt_denoise_temporal): SVGF's reprojection, history and temporal variance (Schied et al. 2017, 4.1 and 4.2).
 * The context keeps the previous call's guide, RayGenerator, colour history (its level 1 output, step 1: SVGF's feedback) and the
 * moments record {mu1, mu2, h, 0}. Per participating pixel p: x_p projected into the previous camera gives storage coordinates
 * (px, pr); its 2 x 2 bilinear taps (order r0x0, r0x1, r1x0, r1x1) that pass dn_temporal_tap_valid form the history; then
 * dn_temporal_integrate. Pixels that do not participate get h = 0 (never a tap of the next call). ---- */
constexpr float DN_TEMPORAL_NORMAL_MIN = 0.9f;  /* a tap needs n_p . n_q >= this */
constexpr float DN_TEMPORAL_PLANE_MAX = 2.0f;   /* ... and |n_p . (x_q - x_p)| <= this * f_p */
constexpr float DN_TEMPORAL_WEIGHT_MIN = 0.01f; /* history exists if the valid taps' bilinear weights sum to >= this */
constexpr float DN_HISTORY_MAX = 32.0f;         /* cap of the history length h */
constexpr float DN_HISTORY_VARIANCE_MIN = 4.0f; /* h >= this: the temporal variance; below: the spatial window (k_denoise_var's) */

/* dn_reproject, the inverse of primary_direction: temporal_reproject.h (shared with the ReSTIR history's gather) */
/* the 2 x 2 taps from (x0, r0), weights in tap order r0x0, r0x1, r1x0, r1x1 */
RT_HD void dn_bilinear(float px, float pr, int& x0, int& r0, float w[4])
{
    const float fx0 = floorf(px), fr0 = floorf(pr);
    const float fx = px - fx0, fr = pr - fr0;
    x0 = (int)fx0;
    r0 = (int)fr0;
    w[0] = (1.0f - fx) * (1.0f - fr);
    w[1] = fx * (1.0f - fr);
    w[2] = (1.0f - fx) * fr;
    w[3] = fx * fr;
}
/* a tap of the previous frame that is inside the image: SURFACE, history length > 0, the same orientation and the same plane */
RT_HD bool dn_temporal_tap_valid(f3 np, f3 xp, float fp, uint32_t word_q, float hq, f3 nq, f3 xq)
{
    return dn_kind(word_q) == DN_KIND_SURFACE && hq > 0.0f && dot(np, nq) >= DN_TEMPORAL_NORMAL_MIN &&
           fabsf(dot(np, xq - xp)) <= DN_TEMPORAL_PLANE_MAX * fp;
}

/* weighted sums over the valid taps in tap order; h of the valid tap with the largest weight (the first on ties) */
struct DnHistory
{
    float sw, r, g, b, m1, m2, wmax, h;
};
RT_HD DnHistory dn_history_init() { return DnHistory{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}; }
RT_HD void dn_history_add(DnHistory& s, float w, float4 c, float4 m)
{
    s.sw = s.sw + w;
    s.r = s.r + w * c.x;
    s.g = s.g + w * c.y;
    s.b = s.b + w * c.z;
    s.m1 = s.m1 + w * m.x;
    s.m2 = s.m2 + w * m.y;
    if (w > s.wmax)
    {
        s.wmax = w;
        s.h = m.z;
    }
}
RT_HD float dn_blend(float prev, float cur, float a) { return (1.0f - a) * prev + a * cur; }
/* the integrated colour {c, 0} and moments {mu1, mu2, h, 0} of a participating pixel with demodulated value e */
RT_HD void dn_temporal_integrate(const DnHistory& s, f3 e, float alpha_c, float alpha_m, float4& col, float4& mom)
{
    const float l = dn_luminance(e);
    col.w = 0.0f;
    mom.w = 0.0f;
    if (!(s.sw >= DN_TEMPORAL_WEIGHT_MIN))
    {
        col.x = e.x;
        col.y = e.y;
        col.z = e.z;
        mom.x = l;
        mom.y = l * l;
        mom.z = 1.0f;
        return;
    }
    const float hn = s.h + 1.0f;
    const float h = hn < DN_HISTORY_MAX ? hn : DN_HISTORY_MAX;
    const float inv = 1.0f / h;
    const float ac = alpha_c > inv ? alpha_c : inv, am = alpha_m > inv ? alpha_m : inv;
    col.x = dn_blend(s.r / s.sw, e.x, ac);
    col.y = dn_blend(s.g / s.sw, e.y, ac);
    col.z = dn_blend(s.b / s.sw, e.z, ac);
    mom.x = dn_blend(s.m1 / s.sw, l, am);
    mom.y = dn_blend(s.m2 / s.sw, l * l, am);
    mom.z = h;
}
/* h >= DN_HISTORY_VARIANCE_MIN: max(0, mu2 - mu1^2) */
RT_HD float dn_temporal_variance(float4 mom)
{
    const float v = mom.y - mom.x * mom.x;
    return v > 0.0f ? v : 0.0f;
}

}  // namespace rt
