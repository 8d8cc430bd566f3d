/*
 * temporal_reproject.h — where the temporal history of a pixel comes from once the camera has moved (rt_temporal_reprojection,
 * DESIGN.md section 13), and the projection it shares with the temporal denoiser.
 *
 * The reference merges pixel p of the current frame with the reservoir pixel p held in the previous frame
 * (10_restir_di.cu:137-237), which is the right history only while the camera stands still. With the mode on, and a history
 * buffer that was written under another RayGenerator than the current one, a shaded pixel projects its surface point into
 * that previous RayGenerator, takes the NEAREST pixel there, and merges that pixel's reservoir — or Reservoir{} where there is
 * none: behind the previous camera, outside its image, NaN / infinite coordinates, or a previous pixel that was sky or
 * emissive (its record's shaded bit is clear). Everything after the choice of the record is temporal_merge as it stands
 * (frame_kernels.h): the random number is keyed by the CURRENT pixel and drawn either way, the rejection heuristics see the
 * gathered record's origin position / normal, the shadowed target function's ray goes to the gathered sample.
 *
 * Not followed here: geometry moved by rt_scene_update. The reprojection uses the two cameras only, so the history of a surface
 * that moved is looked up where the surface is NOW, and meets the rejection heuristics exactly as it does with the mode off.
 * rt_temporal_motion (temporal_motion.h) follows it, on top of this header.
 *
 * RT_HD functions over IEEE +, -, *, / and the correctly rounded square root of rt_device.h: compiled by hipcc and by
 * `g++ -ffp-contract=off` they give the same bits, so the CPU restatement (tests/temporal_reproject_ref.py) picks the
 * pixel the kernels pick. No index is formed from a value that has not passed the float range test first.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

/* inverse of primary_direction (frame_kernels.h: pixel x has u = x / W, storage row = H - 1 - yi with v = yi / H) for the
 * RayGenerator {o, R, U} (R, U and forward = normalize(U x R) orthogonal, as raygen_lookat makes them): continuous storage
 * coordinates of x. false behind the camera, or where no bilinear tap can be inside the image (NaN included) */
RT_HD bool dn_reproject(f3 x, f3 o, f3 R, f3 U, int W, int H, float& px, float& pr)
{
    const f3 fwd = normalize(cross(U, R));
    const f3 d = x - o;
    const float t = dot(d, fwd);
    if (!(t > 0.0f)) return false;
    const float a = dot(d, R) / (t * dot(R, R)), b = dot(d, U) / (t * dot(U, U));
    px = ((a + 1.0f) * 0.5f) * (float)W;
    pr = (float)(H - 1) - ((1.0f - b) * 0.5f) * (float)H;
    return px >= -1.0f && px < (float)W && pr >= -1.0f && pr < (float)H;
}

/* the 36 bytes of two RayGenerators {origin, right, up} are the same (bit patterns: -0 is not +0, a NaN equals itself) */
RT_HD bool tr_same_camera(const float* a, const float* b)
{
    bool same = true;
    for (int i = 0; i < 9; ++i) same = same && pm_f2u(a[i]) == pm_f2u(b[i]);
    return same;
}

/* the previous frame's pixel that saw surface point sp: storage coordinates (xq, rq), meaningful only where valid */
struct TrPixel
{
    bool valid;
    int xq, rq;
};
RT_HD TrPixel tr_previous_pixel(f3 sp, f3 o, f3 R, f3 U, int W, int H)
{
    TrPixel q;
    q.valid = false;
    q.xq = 0;
    q.rq = 0;
    float px = 0.0f, pr = 0.0f;
    /* t > 0, and (px, pr) inside [-1, W) x [-1, H): whatever fails that (NaN, infinity) has no nearest pixel either */
    if (!dn_reproject(sp, o, R, U, W, H, px, pr)) return q;
    const float fx = floorf(px + 0.5f), fr = floorf(pr + 0.5f);
    /* decided in float: only values this test has passed are converted */
    if (!(fx >= 0.0f && fx < (float)W && fr >= 0.0f && fr < (float)H)) return q;
    q.valid = true;
    q.xq = (int)fx;
    q.rq = (int)fr;
    return q;
}

}  // namespace rt
