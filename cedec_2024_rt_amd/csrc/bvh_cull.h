/*
 * bvh_cull.h — what decides whether a walk of the 4-wide quantised tree (bvh.h) enters a child box: the quantiser that
 * writes the byte planes and the slab test that reads them. RT_HD, so hipcc and a plain g++ compile the same expressions:
 * tests/test_targeted_rays_cpu.py runs them on the host against intersect_ray_triangle (rt_device.h), and
 * tests/test_gpu_targeted_rays.py runs every walk on rays aimed at vertices, edges, box faces and duplicated triangles.
 *
 * THE CLAIM. A walk returns what brute force over all triangles returns iff no box is culled whose subtree holds a triangle
 * that intersect_ray_triangle, AS IT COMPUTES IN BINARY32, accepts with a t that can still win (t <= best, "=" included: the
 * later index wins at equal t). Three margins keep such a box; none of them does alone. u = 2^-24, R = the largest
 * |coordinate| of the scene.
 *
 * (1) The build's pad. Every leaf box is the triangle's (or fragment's) box grown by P = 4e-5 * max(1, R) on every side
 *     (restir_rt.hip where the builds compute it, bvh_refit.h::refit_pad), about 670 u R, and inner boxes hold their children.
 *     It is there because of what the intersector accepts: tc = fl(dot(v0 - ro, n) / dot(n, rd)), pc = fl(ro + rd * tc),
 *     tmin <= tc <= tmax and three edge functions a_i = fl(n . (e_i x (pc - v_i))) >= 0. a_i is |n||e_i| times the distance
 *     of pc's projection from edge i and carries about 7u |n||e_i||pc - v_i| of rounding, so pc may lie a few u R outside
 *     an edge, whatever the triangle's shape (one so thin that fl(n) has lost its direction is outside this argument); and
 *     the point of the ray at tc is off the triangle's plane by a few u |v0 - ro| (the 1 / |n . rd| of a grazing ray cancels
 *     when the error of t is turned back into a distance).
 * (2) The quantiser only moves planes outward: fl(origin + q * scale), the plane a walk decodes, is outside the child box.
 * (3) The relative pad of the test, WIDE_SLAB_PAD. t(q) = fma(q, B, A) with A = (origin - ro) * inv and B = scale * inv
 *     (exact: a power of two) carries 2u |A| from A and u |t(q)| of its own. Seen from far away (|ro| >> R) A and t(q) are
 *     both about t, the error is relative, and 2^-20 = 16u covers it together with the few u of tc itself. Seen from
 *     nearby, A and q * B can cancel: at a tile vertex seen from nearly above, |A_x| = |origin_x - ro_x| / |rd_x| is 1e3 t
 *     and the error of t(q), u |A_x|, is 1e-3 of t: no relative pad covers that. In position it is u |origin_x - ro_x|,
 *     and it is large against t only where ro_x is nearer to the plane than to the record's origin, so it is at most the
 *     record's extent times u, below 2u R: P of (1) covers it 300 times over. Without P the same test loses 0.1 % of the
 *     hits at tile vertices and edges (tests/test_targeted_rays_cpu.py asserts that it does: the rays of these tests reach
 *     the place where a cull goes wrong).
 * (4) The accepted set. The intersector's own range test gives tmin <= tc <= tmax and a hit that can still win has
 *     tc <= best, so with tn <= tc <= tf from (1)-(3) the box passes max(tn, tmin) <= min(tf, best) * PAD, for best = tmax
 *     and for best = tc of an equal hit alike.
 * What this does NOT bound: P grows with R and not with |ro|, and (1) needs a few u (|ro| + R). The relative pad takes the
 * part that grows with t, and on the rays of the tests (origins up to 1e3 from scenes of extent 8e-3 to 1e5; on the host up
 * to 1e7) nothing is lost, but there is no proof for an origin a million scene sizes away.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

/* Quantisation of one inner record, shared by every writer of the records (bvh_build_host.h::collapse_wide,
 * bvh_build_device.h::k_collapse_level, bvh_refit.h::k_refit_level). wide_quant_scale: per axis the power-of-two step
 * whose 255 steps cover the node box [lo, hi], exponent clamped to the normal range; returns ex | ey << 8 | ez << 16.
 * wide_quant_child: child k's byte bounds in q (q[a] = lo bytes, q[3 + a] = hi bytes), rounded outward so that the
 * box the traversal decodes in binary32, lo + q * scale, contains the child box. */
RT_HD uint32_t wide_quant_scale(const float lo[3], const float hi[3], float scale[3])
{
    uint32_t ebits = 0;
    for (int a = 0; a < 3; ++a)
    {
        const float ext = fmaxf(hi[a] - lo[a], 1e-30f);
        int e;
        frexpf(ext / 255.0f, &e); /* ext/255 = m * 2^e, m in [0.5,1) => 2^e >= ext/255 */
        int biased = e + 127;
        if (biased < 1) biased = 1;
        if (biased > 254) biased = 254;
        ebits |= (uint32_t)biased << (8 * a);
        scale[a] = ldexpf(1.0f, biased - 127);
    }
    return ebits;
}
RT_HD void wide_quant_child(const float lo[3], const float scale[3], const float clo[3], const float chi[3], int k, uint32_t q[6])
{
    for (int a = 0; a < 3; ++a)
    {
        int ql = (int)floorf((clo[a] - lo[a]) / scale[a]);
        int qh = (int)ceilf((chi[a] - lo[a]) / scale[a]);
        while (ql > 0 && lo[a] + (float)ql * scale[a] > clo[a]) --ql;
        while (qh < 255 && lo[a] + (float)qh * scale[a] < chi[a]) ++qh;
        ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql);
        qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
        q[a] |= (uint32_t)ql << (8 * k);
        q[3 + a] |= (uint32_t)qh << (8 * k);
    }
}

/* (3) above: [tn, tf] is accepted iff max(tn, tmin) <= min(tf, best) * PAD. PAD >= (1 + 4e-7) / (1 - 4e-7), the margins r01-r03
 * put on both ends (tn * (1 - 4e-7) <= tf * (1 + 4e-7)): whatever that test kept this one keeps (tmin, best >= 0) */
constexpr float WIDE_SLAB_PAD = 1.0f + 0x1p-20f;

RT_HD float wide_scale(uint32_t ebits, int a) { return as_float(((ebits >> (8 * a)) & 0xffu) << 23); }
RT_HD float wide_byte(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xffu); }

/* THE accept predicate of every wide walk, for children 0 .. N-1 of one record (N = 4; N = 1: the walk that gives each child a
 * lane of its own passes the words shifted down to its child).
 *   ox, oy, oz, ebits: the record's first quad { origin.xyz, bits(ex | ey << 8 | ez << 16) }; n*: the words of the byte planes
 *   the ray enters through on each axis (the low planes for inv >= 0, else the high ones: t(q) is monotone in q with the sign
 *   of B), f*: of those it leaves through; inv: 1 / rd clamped to +-1e30 (finite: an exactly axis-parallel ray must still be
 *   culled by its slab); [tmin, best]: what is left of the ray.
 *   tn[k]: the entry distance the closest-hit walks order the children by; h[k]: child k's box is kept.
 * t(q) = (origin + q * scale - ro) * inv = A + q * B: one FMA per plane. Rounding may leave tn a few 1e-7 too large and tf too
 * small; one factor on the far side covers both. */
template <int N>
RT_HD void wide_accept(float ox, float oy, float oz, uint32_t ebits, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t fx, uint32_t fy,
                       uint32_t fz, f3 ro, f3 inv, float tmin, float best, float tn[N], bool h[N])
{
    const float Ax = (ox - ro.x) * inv.x, Ay = (oy - ro.y) * inv.y, Az = (oz - ro.z) * inv.z;
    const float Bx = wide_scale(ebits, 0) * inv.x, By = wide_scale(ebits, 1) * inv.y, Bz = wide_scale(ebits, 2) * inv.z;
    for (int k = 0; k < N; ++k)
    {
        const float n = fmaxf(fmaxf(__builtin_fmaf(wide_byte(nx, k), Bx, Ax), __builtin_fmaf(wide_byte(ny, k), By, Ay)),
                              __builtin_fmaf(wide_byte(nz, k), Bz, Az));
        const float f = fminf(fminf(__builtin_fmaf(wide_byte(fx, k), Bx, Ax), __builtin_fmaf(wide_byte(fy, k), By, Ay)),
                              __builtin_fmaf(wide_byte(fz, k), Bz, Az));
        tn[k] = fmaxf(n, tmin);
        h[k] = tn[k] <= fminf(f, best) * WIDE_SLAB_PAD;
    }
}

} // namespace rt
