/*
 * temporal_unbiased.h — the temporal merge with the 1/Z normalisation for a history that comes from ANOTHER pixel
 * (rt_temporal_unbiased), on top of temporal_reproject.h.
 *
 * The reference's merge (10_restir_di.cu:137-237) normalises by 1/M and counts the history's M whether or not the history's pixel
 * could have produced the selected sample. That is unbiased while the history is the pixel's own; once rt_temporal_reprojection
 * gathers it from the previous frame's pixel that saw the surface point, the two supports differ at every contact shadow and depth
 * edge: a sample the previous pixel could never have held (behind its surface, or occluded from it under visibility reuse) is
 * divided by an M that includes the previous pixel's count, and the image darkens, more with every frame of a moving camera.
 *
 * Here the merge chain is the reference's (same draw, same rejection heuristics, same cap), and afterwards the history is asked
 * whether its own target function is positive at the selected sample y: geometry term > 0 from ITS surface (the record's origin)
 * and, under visibility reuse, y visible from there — known from the record's flag if y is the history's own sample, one shadow ray
 * from the history's origin otherwise. Z = the candidates' M (their source reaches every light point) + the history's scaled M if
 * it says yes. If the history's sample won, the ray from the pixel's OWN surface is walked here too, so that the stored flag means
 * "visible from the pixel that wrote the record" again, and the record's origin is the writer's surface whoever the sample came from.
 *
 * Function templates over a record type R with the fields {hit_p, hit_n, org_p, org_n: f3; lum, ucw, w_sum: float; M: int; vis: bool}
 * (the kernels' Res; the CPU restatement's own struct), RT_HD over IEEE +, -, *, / in this order: compiled by hipcc and by
 * `g++ -ffp-contract=off` they give the same bits (tests/temporal_unbiased_ref.py). The rays are the caller's: the kernel walks the
 * BVH between the two halves (frame_kernels.h, k_temporal_unbiased), the restatement tests every triangle.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

struct TuChain
{
    int Mk;         /* the history's M after the cap and the rejection heuristics */
    int Z;          /* the candidates' M: what is in Z whatever the history says */
    bool from_hist; /* the history's sample was selected */
};

/* first half: the merge chain. r = the pixel's candidates, pr = the gathered history (all zero where there is none), u = the
 * pixel's draw (drawn either way). Leaves r.org_* alone (the second half sets them) and caps pr.M in place. */
template <class R>
RT_HD TuChain tu_merge_chain(R& r, R& pr, f3 sp, f3 sn, f3 eye, int ris_sample_count, bool vis_reuse, float u)
{
    TuChain c;
    const int cap = 20 * ris_sample_count;
    pr.M = pr.M < cap ? pr.M : cap;
    c.Mk = scale_M(pr.M, rejection_heuristics(r.org_p, r.org_n, pr.org_p, pr.org_n, eye));
    float p_hat_y = target_unshadowed(sp, sn, pr.hit_p, pr.hit_n, pr.lum);
    if (vis_reuse) p_hat_y *= pr.vis ? 1.0f : 0.0f;
    const float weight = p_hat_y * pr.ucw * (float)c.Mk;
    c.Z = r.M;
    r.w_sum += weight;
    r.M += c.Mk;
    c.from_hist = reservoir_accept(u, weight, r.w_sum);
    if (c.from_hist)
    {
        r.hit_p = pr.hit_p; r.hit_n = pr.hit_n; r.lum = pr.lum; r.vis = pr.vis;
    }
    return c;
}

/* between the halves: does geometry alone let the history's pixel produce the selected sample? (false without a history: Mk = 0) */
template <class R>
RT_HD bool tu_hist_geometry(const TuChain& c, const R& r, const R& pr) { return c.Mk > 0 && unbiased_in_support(pr.org_p, pr.org_n, r.hit_p, r.hit_n); }
/* the rays the second half wants answered: history origin -> y (at most this one from a surface other than the pixel's own) ... */
RT_HD bool tu_needs_hist_ray(const TuChain& c, bool in_geo, bool vis_reuse) { return in_geo && vis_reuse && !c.from_hist; }
/* ... and own surface -> y, the ray resolve would walk: only where the history's sample won */
RT_HD bool tu_needs_own_ray(const TuChain& c, bool vis_reuse) { return vis_reuse && c.from_hist; }

/* second half. hist_visible / own_visible: the answers of the two rays, read only where tu_needs_* asked for them. Returns whether
 * the history's M went into Z. */
template <class R>
RT_HD bool tu_finish(R& r, const R& pr, const TuChain& c, bool in_geo, bool vis_reuse, bool hist_visible, bool own_visible, f3 sp, f3 sn)
{
    bool in = in_geo;
    if (in && vis_reuse) in = c.from_hist ? pr.vis : hist_visible;
    const int Z = c.Z + (in ? c.Mk : 0);
    if (tu_needs_own_ray(c, vis_reuse)) r.vis = own_visible;
    r.org_p = sp;
    r.org_n = sn;
    r.ucw = unbiased_ucw(r.w_sum, Z, target_unshadowed(sp, sn, r.hit_p, r.hit_n, r.lum));
    return in;
}

}  // namespace rt
