/*
 * neighbour_pick.h — the one owner of the spatial pass's neighbour pick (common/reservoir.hpp:89-95 + 10_restir_di.cu:305-325):
 * two uniform draws -> a Gaussian offset (Box-Muller) -> the neighbour's integer pixel (nx, ny).
 *
 *   neighbour_pick_exact   the reference's expressions over portable_math.h, operation for operation: what every replay of the
 *                          pick computes (k_spatial, k_spatial_unbiased, k_halo_mark, k_spatial_bytes, the oracle).
 *   neighbour_pick         (device) the same two integers from the hardware's log2 / sqrt / sin / cos, behind an interval guard;
 *                          lanes the guard cannot clear ("near ties") take neighbour_pick_exact. k_spatial_coop calls this one.
 *
 * WHY THE INTEGERS ARE THE SAME. The floats of the pick (radius, sin, cos, gx, gy) feed nothing but
 *     nx = f2i_sat((float)x + sx),  sx = scale * gx        (ny likewise from yi and sy)
 * so bit-exactness binds (nx, ny) only. Let sx' be the fast value and E a bound with |sx' - sx| <= E, sx being what the exact
 * code computes, roundings included. Then, in real numbers, sx' - E <= sx <= sx' + E; rounding to nearest is monotone and sx is a
 * binary32 number, so lo = RN(sx' - E) <= sx <= RN(sx' + E) = hi; binary32 addition of a fixed (float)x is monotone, and so is
 * the float -> int conversion on numbers (truncation, saturating). Hence
 *     f2i_sat((float)x + lo) <= nx <= f2i_sat((float)x + hi)
 * and where the two ends agree, nx is that integer. This covers the float -> int seam itself (at x = 1900 .. 3800 one unit in the
 * last place of the sum is 1.2e-4 .. 2.4e-4, more than E): no distance-to-integer reasoning is involved. NaN is the one value the
 * conversion does not order (it gives 0), so a lane whose fast values are not finite fails the guard outright; rv0 = 0 is such a
 * lane (log2 -> -inf).
 *
 * WHERE E COMES FROM. Both draws are k * 2^-23, k = 0 .. 2^23 - 1 (rt_device.h, PCG::uniformf), so the fast functions were
 * compared with the exact ones over EVERY input on the MI355X (tools/pick_error_sweep.py, docs/MEASUREMENT_LOG_r22.md):
 *     Er = max |radius' - radius|  over rv0,    Es, Ec = max |sin' - sin|, |cos' - cos|  over rv1,    Em = max(Es, Ec),
 *     Rmax = the largest finite radius = sqrt(2 ln 2^23) = 5.6467.
 * With r' = r + dr, c' = c + dc, |dr| <= Er, |dc| <= Em, |c| <= 1, r <= Rmax:
 *     |r' c' - r c| <= Er + Rmax Em + Er Em
 *     gx' = RN(r' c'), gx = RN(r c): two roundings of numbers below 8, each <= 2^-22
 *         => |gx' - gx| <= Eg = Er + Rmax Em + Er Em + 2^-21
 *     sx' = RN(scale gx'), sx = RN(scale gx): two roundings, each <= 2^-24 |scale| (Rmax + Eg)
 *         => |sx' - sx| <= |scale| (Eg + 2^-23 (Rmax + Eg))
 * The committed constants are the measured maxima DOUBLED (the sweep is exhaustive, so the margin is against a mistake in this
 * composition, not against sampling), and the rounding terms are doubled with them:
 *     E = |scale| * kPickK,   kPickK = kPickEr + kPickRmax kPickEm + kPickEr kPickEm + 2^-20 + 2^-22 (kPickRmax + 1).
 * E follows the radius of the options (scale = spatial_radius / 1.96); nothing here is fixed for radius 30.
 * The maxima belong to gfx950's instructions: a build for another GPU reruns the sweep before it trusts these constants.
 *
 * Dual-use like portable_math.h: hipcc (device + host pass) and plain C++ on the host, where only the exact function and the
 * guard exist (tests/test_neighbour_pick_cpu.py drives the guard with adversarial offsets).
 */
#pragma once
#include "rt_device.h"

namespace rt
{

/* today's expressions, moved verbatim: same operations, same order [parity] */
RT_HD void neighbour_pick_exact(float rv0, float rv1, int x, int yi, float scale, int* nx, int* ny)
{
    /* common/reservoir.hpp:89-95 with portable log/cos/sin */
    const float radius = sqrt_guarded(fmax_dev(-2.0f * pm_logf(rv0), 0.0f));
    const float phi = 2.0f * kPI * rv1;
    float sn_phi, cs_phi;
    pm_sincosf(phi, &sn_phi, &cs_phi);
    const float gx = radius * cs_phi, gy = radius * sn_phi;
    *nx = f2i_sat((float)x + scale * gx);
    *ny = f2i_sat((float)yi + scale * gy);
}

/* the measured maxima, rounded up and doubled (docs/MEASUREMENT_LOG_r22.md section 2: Er 4.768e-07 at rv0 = 4 * 2^-23, Es 4.619e-07,
 * Ec 4.172e-07, Rmax 5.646660 at rv0 = 2^-23) */
constexpr float kPickEr = 2.0f * 4.77e-07f;
constexpr float kPickEm = 2.0f * 4.62e-07f;
constexpr float kPickRmax = 5.6467f; /* the sweep's largest finite radius, rounded up: sqrt(2 ln 2^23) = 5.64666 */
constexpr float kPickK = kPickEr + kPickRmax * kPickEm + kPickEr * kPickEm + 9.5367431640625e-07f /* 2^-20 */ + 2.384185791015625e-07f /* 2^-22 */ * (kPickRmax + 1.0f);

/* the bound on |sx' - sx| and |sy' - sy| for this scale */
RT_HD float neighbour_pick_bound(float scale) { return fabsf(scale) * kPickK; }

/* The guard. sx, sy: values within E of the exact scale * gx, scale * gy. True: (*nx, *ny) are the exact integers. False: near a
 * tie, or not finite (|sx| + |sy| is then inf or NaN and the comparison fails): (*nx, *ny) mean nothing. */
RT_HD bool neighbour_pick_guard(float sx, float sy, float E, int x, int yi, int* nx, int* ny)
{
    const float fx = (float)x, fy = (float)yi;
    const int x_lo = f2i_sat(fx + (sx - E)), x_hi = f2i_sat(fx + (sx + E));
    const int y_lo = f2i_sat(fy + (sy - E)), y_hi = f2i_sat(fy + (sy + E));
    *nx = x_lo;
    *ny = y_lo;
    return (x_lo == x_hi) & (y_lo == y_hi) & (fabsf(sx) + fabsf(sy) < 1.0e30f) & (E >= 0.0f);
}

#if defined(__HIPCC__)
/* the hardware's transcendentals: log2 (v_log_f32), sqrt (v_sqrt_f32), sin / cos of an angle in REVOLUTIONS (v_sin_f32 /
 * v_cos_f32: the draw itself, no 2 pi and no range reduction). Named for the device pass only, as hw_rcp / hw_sqrt are. */
#if defined(__HIP_DEVICE_COMPILE__)
RT_DEV float hw_log2(float x) { return __builtin_amdgcn_logf(x); }
RT_DEV float hw_sin_rev(float x) { return __builtin_amdgcn_sinf(x); }
RT_DEV float hw_cos_rev(float x) { return __builtin_amdgcn_cosf(x); }
#else
RT_DEV float hw_log2(float x) { return log2f(x); }
RT_DEV float hw_sin_rev(float x) { return sinf(6.2831853f * x); }
RT_DEV float hw_cos_rev(float x) { return cosf(6.2831853f * x); }
#endif
/* radius' ~ sqrt(-2 ln rv0) = sqrt(log2(rv0) * (-2 ln 2)); rv0 in (0, 1): the product is >= 0, no clamp needed (rv0 = 0 gives
 * +inf and fails the guard) */
RT_DEV float neighbour_pick_fast_radius(float rv0) { return hw_sqrt(hw_log2(rv0) * -1.3862943611198906f); }
/* fast path + guard for one lane */
RT_DEV bool neighbour_pick_fast(float rv0, float rv1, int x, int yi, float scale, float E, int* nx, int* ny)
{
    const float radius = neighbour_pick_fast_radius(rv0);
    const float sx = scale * (radius * hw_cos_rev(rv1)), sy = scale * (radius * hw_sin_rev(rv1));
    return neighbour_pick_guard(sx, sy, E, x, yi, nx, ny);
}
/* rt_neighbour_pick: what the rounds of k_spatial_coop do */
enum { PICK_EXACT = 0, PICK_FAST = 1, PICK_FORCE_SLOW = 2 };
/* The pick of k_spatial_coop. mode (wave-uniform): PICK_FAST = fast path + guard, PICK_EXACT = the exact function only,
 * PICK_FORCE_SLOW = the guard fails on every lane (the slow path through the same control flow). E = neighbour_pick_bound(scale).
 * Works under any exec mask. Returns whether this lane took the exact function (a near tie, unless mode is PICK_EXACT: the counters of rt_neighbour_pick_stats). */
RT_DEV bool neighbour_pick(int mode, float rv0, float rv1, int x, int yi, float scale, float E, int* nx, int* ny)
{
    bool ok = false;
    if (mode != PICK_EXACT) ok = neighbour_pick_fast(rv0, rv1, x, yi, scale, E, nx, ny);
    if (mode == PICK_FORCE_SLOW) ok = false;
    if (__ballot(!ok) != 0) /* a wavefront without a near tie never enters */
    {
        if (!ok) neighbour_pick_exact(rv0, rv1, x, yi, scale, nx, ny);
    }
    return !ok;
}
#endif /* __HIPCC__ */

} /* namespace rt */
