/*
 * denoise_antilag.h — how rt_denoise_temporal raises its blend factors where the lighting has changed (rt_denoise_temporal_antilag,
 * DESIGN.md section 19). rt_denoise_temporal blends every frame into its history with alpha = max(alpha, 1 / h): it finds the history
 * (denoise_math.h, denoise_motion.h) and cannot tell that the history no longer describes the light. An adapted call (the toggle on
 * and a history to read) compares, around every participating pixel p that has a history, the current frame with the reprojected
 * history over a window and trusts the frame more the further apart they are.
 *
 * Per pixel q of the call: e_q the demodulated value, c_prev(q) the reprojected colour history (the quotients dn_temporal_integrate
 * forms; under a followed call those of the followed lookup), l_e(q) = dn_luminance(e_q), l_h(q) = dn_luminance(c_prev(q)), and
 * l_h(q) = -1 where q has no history or does not participate. The window of p: |dx|, |dy| <= radius, inside the image, members only
 * (dn_antilag_member: a history of their own, n_p . n_q >= DN_TEMPORAL_NORMAL_MIN on the current guide; p is a member). In window
 * order (dy outer, dx inner, ascending): mc = sum l_e, mh = sum l_h, n = the member count. Then
 *     lambda  = |mc - mh| / (max(mc, mh) + floor * n)          (0 where the denominator is not positive)
 *     lambda' = clamp((lambda - lo) / (hi - lo), 0, 1)
 *     alpha'  = alpha + (1 - alpha) * lambda'                   (colour and moments alike)
 * and dn_antilag_integrate is dn_temporal_integrate's blend with those alphas, its max(., 1 / h) included; h is unchanged. The moments
 * record's fourth component carries lambda' (0 without history, in calls that are not adapted, and with the toggle off).
 *
 * The floor is what keeps a firefly in a dark window (a relative gradient of 1) from resetting the history; it is in units of
 * demodulated luminance per member.
 *
 * RT_HD functions, binary32 in this order; compiled by hipcc and by `g++ -ffp-contract=off` (tests/denoise_antilag_ref.py) they give
 * the same bits.
 */
#pragma once
#include "denoise_math.h"

namespace rt
{

constexpr int DN_ANTILAG_RADIUS_MAX = 4;

/* rt_denoise_antilag_params as the kernels see them */
struct DnAntilag
{
    int radius;
    float lo, hi, floor;
};

/* l_h of a pixel that has a history (the gather pass writes -1 for the others) */
RT_HD bool dn_antilag_has_history(float lh) { return !(lh < 0.0f); }
RT_HD bool dn_antilag_member(f3 np, f3 nq, float lh_q) { return dn_antilag_has_history(lh_q) && dot(np, nq) >= DN_TEMPORAL_NORMAL_MIN; }

/* sums over the members in window order */
struct DnGradient
{
    float mc, mh;
    int n;
};
RT_HD DnGradient dn_gradient_init() { return DnGradient{0.0f, 0.0f, 0}; }
RT_HD void dn_gradient_add(DnGradient& g, float le, float lh)
{
    g.mc = g.mc + le;
    g.mh = g.mh + lh;
    g.n = g.n + 1;
}
RT_HD float dn_gradient_lambda(const DnGradient& g, float floor)
{
    const float d = (g.mc > g.mh ? g.mc : g.mh) + floor * (float)g.n;
    return d > 0.0f ? fabsf(g.mc - g.mh) / d : 0.0f;
}
/* lambda': 0 for a NaN */
RT_HD float dn_antilag_response(float lambda, float lo, float hi)
{
    const float t = (lambda - lo) / (hi - lo);
    return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
}
RT_HD float dn_antilag_alpha(float alpha, float lr) { return alpha + (1.0f - alpha) * lr; }

/* dn_temporal_integrate for a pixel with a history, from what the gather pass kept: cprev = the quotients s.rgb / s.sw,
 * mprev = {s.m1 / s.sw, s.m2 / s.sw, s.h}; lr = lambda'. lr = 0 gives dn_temporal_integrate's bits. */
RT_HD void dn_antilag_integrate(float4 cprev, float4 mprev, f3 e, float alpha_c, float alpha_m, float lr, float4& col, float4& mom)
{
    const float l = dn_luminance(e);
    const float hn = mprev.z + 1.0f;
    const float h = hn < DN_HISTORY_MAX ? hn : DN_HISTORY_MAX;
    const float inv = 1.0f / h;
    const float alc = dn_antilag_alpha(alpha_c, lr), alm = dn_antilag_alpha(alpha_m, lr);
    const float ac = alc > inv ? alc : inv, am = alm > inv ? alm : inv;
    col.x = dn_blend(cprev.x, e.x, ac);
    col.y = dn_blend(cprev.y, e.y, ac);
    col.z = dn_blend(cprev.z, e.z, ac);
    col.w = 0.0f;
    mom.x = dn_blend(mprev.x, l, am);
    mom.y = dn_blend(mprev.y, l * l, am);
    mom.z = h;
    mom.w = lr;
}
/* ... and for a participating pixel without one: dn_temporal_integrate's first branch */
RT_HD void dn_antilag_first(f3 e, float4& col, float4& mom)
{
    const float l = dn_luminance(e);
    col.x = e.x;
    col.y = e.y;
    col.z = e.z;
    col.w = 0.0f;
    mom.x = l;
    mom.y = l * l;
    mom.z = 1.0f;
    mom.w = 0.0f;
}

}  // namespace rt
