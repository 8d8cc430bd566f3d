/*
 * temporal_motion.h — where the temporal history of a pixel comes from once rt_scene_update has moved the triangle it lies on
 * (rt_temporal_motion), on top of temporal_reproject.h, which follows the camera only.
 *
 * The moved range [lo, hi) covers every span given to rt_scene_update since the history buffer was written; tv_prev holds the vertex
 * positions of that time. A shaded pixel whose triangle lies outside the range does what it does without the toggle. A pixel on a
 * triangle inside it carries its Visibility (u, v) back onto the triangle's previous vertices — the expression of surface_info, so a
 * triangle that did not move gives its current surface point bit for bit —, projects that previous point into the previous
 * RayGenerator with tr_previous_pixel (also where the two cameras have the same bytes) and merges the nearest pixel's record, or
 * Reservoir{} under the conditions of temporal_reproject.h. The rejection heuristics are then evaluated in the previous frame:
 * rejection_heuristics(sp_prev, sn_prev, record origin position / normal, eye_prev) asks whether the gathered pixel saw the point
 * this surface point was at. Target function, random number, shadow ray and ucw keep the current surface point.
 *
 * NaN or infinite previous vertices give a NaN or infinite sp_prev, which fails tr_previous_pixel's float range test: Reservoir{},
 * no index. A previously degenerate triangle has a finite sp_prev and a NaN normal: the heuristics' weight is then 0 or NaN and
 * scale_M makes either M = 0.
 *
 * RT_HD functions over the IEEE operations of rt_device.h, binary32 in this order; compiled by hipcc and by `g++ -ffp-contract=off`
 * (tests/temporal_motion_ref.py) they give the same bits. tm_previous_surface is also what a denoiser history that follows moved
 * geometry would start from.
 */
#pragma once
#include "temporal_reproject.h"

namespace rt
{

/* triangle `prim` of a shaded pixel (>= 0) lies in the moved range */
RT_HD bool tm_in_range(int prim, uint32_t lo, uint32_t hi) { return prim >= 0 && (uint32_t)prim >= lo && (uint32_t)prim < hi; }

/* common/core.hpp:189-207 on the previous vertices (v0, v1, v2) and the previous eye */
struct TmSurface
{
    f3 p, n;
};
RT_HD TmSurface tm_previous_surface(f3 v0, f3 v1, f3 v2, float u, float v, f3 eye_prev)
{
    TmSurface s;
    s.p = (1.0f - u - v) * v0 + u * v1 + v * v2;
    s.n = tri_normal(v0, v1, v2);
    const f3 view = normalize(eye_prev - s.p);
    if (dot(view, s.n) < 0.0f) s.n = -s.n;
    return s;
}

}  // namespace rt
