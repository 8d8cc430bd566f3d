/*
 * light_follow.h — carrying the light sample of a ReSTIR history record along with the emissive triangle it lies on when
 * rt_scene_update moves that triangle (rt_temporal_light_motion).
 *
 * A record stores its sample as a world-space point, a normal, a luminance and (side record) a radiance. The candidates' kernel
 * writes them from the light table bit for bit: hit_n = tri_normal(v0, v1, v2), radiance = Ke, lum = luminance(Ke) and
 * hit_p = (1 - bx - by) v0 + bx v1 + by v2. At the moment of an update the old triangles are still there, so the triangle a sample
 * lies on is found again (lf_locate_test, for every old emissive triangle of the updated span; the smallest plane distance wins,
 * then the lowest index: a total order, so the visit order does not matter) and the sample is carried by its barycentrics onto the
 * triangle's new vertices (lf_apply).
 *
 * Locate accepts old triangle t iff
 *   Ke_old(t) has a positive component and the bytes of the record's radiance, tri_normal(t) has the bytes of hit_n (exact equality
 *     is what the candidates' kernel guarantees, and it makes a match on other geometry practically impossible),
 *   t is not degenerate: |e1 x e2| is finite and non-zero,
 *   |n . (hit_p - v0)| <= LF_TAU_P * the largest |vertex coordinate| of t,
 *   the barycentrics of hit_p, u = (d22 dp1 - d12 dp2) / det and v = (d11 dp2 - d12 dp1) / det over the dot products of
 *     e1 = v1 - v0, e2 = v2 - v0, d = hit_p - v0, satisfy u, v >= -LF_TAU_B and u + v <= 1 + LF_TAU_B.
 * Apply, for the located triangle's new 60 bytes: equal to the old 60 bytes, the record keeps every byte; non-emissive, degenerate
 * or not finite, the record becomes Reservoir{} (its shaded bit kept); otherwise hit_p' = (1 - u - v) v0' + u v1' + v v2'
 * (surface_info's expression), hit_n' = tri_normal' (k_light_table's), lum' = luminance(Ke'), radiance = Ke' and
 * ucw' = ucw * (|e1' x e2'| / |e1 x e2|), the Jacobian of carrying a point by its barycentrics (1 up to rounding for a rigid move;
 * without it a light that grows or shrinks biases the merge). M, w_sum, the origin and the visibility bit stay (a stale flag is what
 * every record carries after an update, section 14); the side record's own-visibility word becomes 0, "nothing known".
 *
 * THE TOLERANCES ARE MEASURED (docs/MEASUREMENT_LOG_r32.md; tests/test_light_follow_cpu.py::test_tolerances_are_eight_times_the_measured
 * measures them again): over every sample the oracle's generate_candidate leaves in 8 frames at 64 x 48 on the lamp room and the quad
 * room, and on copies of both scaled by 1 000 and by 0.001 (110 400 samples),
 *   the largest float64 distance of a sample from its own triangle's plane, over the triangle's largest |coordinate|, is 1.187e-7
 *     (between 1.110e-7 and 1.187e-7 on the six scenes: it is relative; the binary32 expression below gives the same figures);
 *   the largest float64 barycentric excess max(-u, -v, u + v - 1) is 0: no sample of these frames lies within rounding of an edge.
 *     What can put a sample that does lie on an edge outside is the binary32 solve below: its largest difference from the float64
 *     solve in u, v or u + v is 3.760e-7 (2.604e-7 to 3.760e-7 on the six scenes). The barycentric figure is the larger of the two.
 * The constants are 8 x these, rounded up to two digits. A point accepted with them lies within LF_TAU_B x the longest edge
 * (<= 6.2e-6 R, R = the scene's largest |coordinate|) of its triangle and LF_TAU_P R of its plane, inside the 4e-5 max(1, R) by which
 * every leaf box of the wide tree is padded (bvh_cull.h): what light_follow_kernels.h's point query relies on.
 *
 * RT_HD functions over the IEEE operations of rt_device.h, binary32 in this order; compiled by hipcc (light_follow_kernels.h) and by
 * `g++ -ffp-contract=off` (tests/light_follow_ref.py) they give the same bits.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

constexpr float LF_TAU_P = 9.5e-7f; /* 8 x 1.187e-7 */
constexpr float LF_TAU_B = 3.1e-6f; /* 8 x 3.760e-7 */

RT_HD bool lf_same_bits(f3 a, f3 b) { return pm_f2u(a.x) == pm_f2u(b.x) && pm_f2u(a.y) == pm_f2u(b.y) && pm_f2u(a.z) == pm_f2u(b.z); }
RT_HD bool lf_emissive(f3 ke) { return ke.x > 0.0f || ke.y > 0.0f || ke.z > 0.0f; } /* 10_restir_di.cpp:196-205 */
RT_HD bool lf_finite(float x) { return (pm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
RT_HD bool lf_finite3(f3 a) { return lf_finite(a.x) && lf_finite(a.y) && lf_finite(a.z); }
RT_HD float lf_max3(float a, float b, float c) { return fmax_dev(fmax_dev(a, b), c); }
/* the largest |coordinate| of three points (a triangle, or two box corners and one of them again) */
RT_HD float lf_max_abs(f3 a, f3 b, f3 c)
{
    return lf_max3(lf_max3(fabsf(a.x), fabsf(a.y), fabsf(a.z)), lf_max3(fabsf(b.x), fabsf(b.y), fabsf(b.z)), lf_max3(fabsf(c.x), fabsf(c.y), fabsf(c.z)));
}
/* the tolerance of a plane distance on triangle (v0, v1, v2); of a box test in a tree whose root box has corners lo, hi */
RT_HD float lf_eps_tri(f3 v0, f3 v1, f3 v2) { return LF_TAU_P * lf_max_abs(v0, v1, v2); }
RT_HD float lf_eps_box(f3 lo, f3 hi) { return LF_TAU_P * lf_max_abs(lo, hi, hi); }

/* |e1 x e2| (twice the area) of a triangle; usable iff finite and non-zero */
RT_HD float lf_area2(f3 v0, f3 v1, f3 v2) { return length(cross(v1 - v0, v2 - v0)); }
RT_HD bool lf_area_ok(float a2) { return lf_finite(a2) && a2 > 0.0f; }

struct LfMatch
{
    bool ok;
    float dist, u, v, area2;
};
/* does the sample (hit_p, hit_n, rad) lie on the old triangle (v0, v1, v2, ke)? */
RT_HD LfMatch lf_locate_test(f3 hit_p, f3 hit_n, f3 rad, f3 v0, f3 v1, f3 v2, f3 ke)
{
    LfMatch m;
    m.ok = false; m.dist = 0.0f; m.u = 0.0f; m.v = 0.0f; m.area2 = 0.0f;
    if (!lf_emissive(ke) || !lf_same_bits(ke, rad)) return m;
    const f3 e1 = v1 - v0, e2 = v2 - v0;
    const f3 c = cross(e1, e2);
    const float a2 = length(c);
    if (!lf_area_ok(a2)) return m;
    const f3 n = c / a2; /* tri_normal(v0, v1, v2): normalize(cross(v1 - v0, v2 - v0)), the same operations */
    if (!lf_same_bits(n, hit_n)) return m;
    const f3 d = hit_p - v0;
    const float dist = fabsf(dot(n, d));
    if (!(dist <= lf_eps_tri(v0, v1, v2))) return m;
    const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), dp1 = dot(d, e1), dp2 = dot(d, e2);
    const float det = d11 * d22 - d12 * d12;
    const float u = (d22 * dp1 - d12 * dp2) / det;
    const float v = (d11 * dp2 - d12 * dp1) / det;
    if (!(u >= -LF_TAU_B) || !(v >= -LF_TAU_B) || !(u + v <= 1.0f + LF_TAU_B)) return m;
    m.ok = true; m.dist = dist; m.u = u; m.v = v; m.area2 = a2;
    return m;
}
/* the total order of the matches: a replaces best (of triangle best_t, -1 = none yet) */
RT_HD bool lf_better(const LfMatch& a, int a_t, const LfMatch& best, int best_t)
{
    return a.ok && (best_t < 0 || a.dist < best.dist || (a.dist == best.dist && a_t < best_t));
}

/* the light side of a record: q0 = {hit_p, ucw}, q1.xyz = hit_n, q2.w = lum, side record = {radiance, own-visibility word} */
struct LfSample
{
    f3 hit_p, hit_n, rad;
    float ucw, lum;
};
enum LfOutcome { LF_KEEP = 0, LF_MOVED = 1, LF_EMPTIED = 2 };
RT_HD bool lf_same_triangle(const float o[15], const float n[15])
{
    bool same = true;
    for (int k = 0; k < 15; ++k) same = same && pm_f2u(o[k]) == pm_f2u(n[k]);
    return same;
}
/* carries s, located at (u, v) on an old triangle of |e1 x e2| = area2_old, onto the triangle's new 15 floats. `jacobian` = false is
 * the planted error of tests/test_light_follow_cpu.py (the area factor left out); every caller of the product passes true.
 * LF_KEEP: s untouched (the caller has compared the 60 bytes). LF_EMPTIED: the caller stores Reservoir{}. */
RT_HD LfOutcome lf_apply(LfSample& s, const LfMatch& m, const float o[15], const float n[15], bool jacobian = true)
{
    if (lf_same_triangle(o, n)) return LF_KEEP;
    const f3 v0 = F3(n[0], n[1], n[2]), v1 = F3(n[3], n[4], n[5]), v2 = F3(n[6], n[7], n[8]), ke = F3(n[12], n[13], n[14]);
    if (!lf_emissive(ke) || !lf_finite3(v0) || !lf_finite3(v1) || !lf_finite3(v2) || !lf_finite3(ke)) return LF_EMPTIED;
    const f3 c = cross(v1 - v0, v2 - v0);
    const float a2 = length(c);
    if (!lf_area_ok(a2)) return LF_EMPTIED;
    s.hit_p = (1.0f - m.u - m.v) * v0 + m.u * v1 + m.v * v2;
    s.hit_n = c / a2;
    s.lum = luminance(ke);
    s.rad = ke;
    if (jacobian) s.ucw = s.ucw * (a2 / m.area2);
    return LF_MOVED;
}

}  // namespace rt
