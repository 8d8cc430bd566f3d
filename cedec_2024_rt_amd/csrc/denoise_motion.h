/*
 * denoise_motion.h — where rt_denoise_temporal looks for the history of a pixel once rt_scene_update has moved the triangle it lies
 * on (rt_denoise_temporal_motion), beside temporal_motion.h, which does the same for the ReSTIR history.
 *
 * Without the toggle a participating pixel projects its current surface point x_p into the previous call's RayGenerator and asks of
 * each of the four taps whether it lay on the plane (n_p, x_p): the history follows the camera, and a surface that moved is looked up
 * where it is now. A followed call (dn_motion_followed) differs for the pixels whose triangle lies in the moved range [lo, hi): their
 * lookup point and normal are those of tm_previous_surface on the triangle's previous vertices, with the (u, v) of this call's guide
 * hit and the previous call's eye. dn_reproject and dn_temporal_tap_valid then run on (x_l, n_l), also where the two cameras have the
 * same bytes: "did the previous frame's tap lie on the plane this point was on". f_p stays the current pixel's footprint, as it does
 * for an unmoved surface under a moving camera. Demodulation, integration, variance, levels and output keep the current guide.
 *
 * A triangle of the range that did not move gives x_l == x_p bit for bit (the expression of dn_surface). NaN or infinite previous
 * vertices fail dn_reproject (!(t > 0) or its range test): no history, h = 1. A previously degenerate triangle has a NaN normal and
 * fails n . n' >= 0.9 on every tap.
 *
 * RT_HD functions, binary32 in this order; compiled by hipcc and by `g++ -ffp-contract=off` (tests/denoise_motion_ref.py) they give
 * the same bits.
 */
#pragma once
#include "denoise_math.h"
#include "temporal_motion.h"

namespace rt
{

/* The host's decision, once per call. toggle: rt_denoise_temporal_motion; has_history: a previous call's buffers exist (dt_valid);
 * have_prev: the previous vertices are kept; hist_gen: the geometry generation the denoiser's history was written under; prev_gen: the
 * one the kept vertices describe; cur_gen: the current one. A history older than the kept vertices gets the camera only. */
RT_HD bool dn_motion_followed(bool toggle, bool has_history, bool have_prev, uint64_t hist_gen, uint64_t prev_gen, uint64_t cur_gen)
{
    return toggle && has_history && have_prev && hist_gen == prev_gen && prev_gen != cur_gen;
}

/* the lookup point and normal of a participating pixel on triangle dn_tri(word) of the range: (v0, v1, v2) its previous vertices */
RT_HD void dn_motion_lookup(f3 v0, f3 v1, f3 v2, float u, float v, f3 eye_prev, f3& xl, f3& nl)
{
    const TmSurface s = tm_previous_surface(v0, v1, v2, u, v, eye_prev);
    xl = s.p;
    nl = s.n;
}

}  // namespace rt
