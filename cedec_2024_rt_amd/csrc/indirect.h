/*
 * indirect.h — rt_indirect: the start of an indirect path, which the kernels (frame_kernels.h, k_indirect
 * through indirect_begin) and the CPU restatement (tests/indirect_ref.py) share, binary32 in this order, no FMA
 * contraction. The depth loop itself is not here: the kernels run path_bounce<8, false> (frame_kernels.h), the restatement states
 * 08_nee's loop on its own.
 *
 * 08_nee's radiance at a pixel is  emission seen directly + next-event term at depth 0 + the next-event terms at depth >= 1
 * (examples/08_nee/08_nee.cu:39-118). The ReSTIR frame estimates the first two at the primary hit; the pass adds the third: a path that
 * starts at the G-buffer's surface with 08_nee's own random stream for the pixel, after the three draws 08_nee spends on its depth-0
 * light sample, and then runs 08_nee's depth loop from depth 1.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

/* common/core.hpp:76-89 with portable cos/sin [parity] */
RT_HD f3 sample_hemisphere(float r0, float r1, float r2)
{
    const float theta = r0 * 2.0f * kPI;
    float radius = r1 + r2;
    if (1.0f < radius) radius = 2.0f - radius;
    float sn_t, cs_t;
    pm_sincosf(theta, &sn_t, &cs_t);
    const float x = cs_t * radius;
    const float z = sn_t * radius;
    const float a = 1.0f - radius * radius;
    const float y = sqrtf((a < 0.0f) ? 0.0f : a);
    return F3(x, y, z);
}

/* common/core.hpp:216-235: the local direction wl in the basis of the surface normal sn and the triangle's first edge [parity] */
RT_HD f3 bounce_direction(f3 v0, f3 v1, f3 sn, f3 wl)
{
    const f3 tg = normalize(v1 - v0);
    const f3 bt = normalize(cross(tg, sn));
    return wl.x * tg + wl.y * sn + wl.z * bt;
}

/* a path as it enters depth 1 of 08_nee's loop */
struct IndirectStart
{
    f3 ro, rd, throughput;
    PCG rng;
};
/* (x, yi): the pixel as the reference numbers it (yi = H - 1 - storage row); sp, sn: the primary hit's point and normal; kd, v0, v1:
 * colour and first edge of the primary triangle */
RT_HD IndirectStart indirect_start(int x, int yi, int frame, f3 sp, f3 sn, f3 kd, f3 v0, f3 v1)
{
    IndirectStart s;
    s.rng = pcg_init(hashPCG3((uint32_t)x, (uint32_t)yi, (uint32_t)frame), 0); /* 08_nee.cu:27 */
    /* 08_nee's depth-0 light sample: three draws (:67-69); the frame's reservoir stands for that term */
    s.rng.uniform();
    s.rng.uniform();
    s.rng.uniform();
    const float r0 = s.rng.uniformf();
    const float r1 = s.rng.uniformf();
    const float r2 = s.rng.uniformf();
    s.rd = bounce_direction(v0, v1, sn, sample_hemisphere(r0, r1, r2));
    s.throughput = F3(1.0f, 1.0f, 1.0f) * kd;
    s.ro = sp + 0.001f * sn;
    return s;
}

}  // namespace rt
