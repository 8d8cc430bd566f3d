/*
 * light_follow_kernels.h — rt_temporal_light_motion on the device (light_follow.h has the rule): one pass over
 * a reservoir buffer inside rt_scene_update, while the old triangles and the old, not yet refitted wide tree are still in place.
 *
 *   k_light_follow_box: the bounding box of the span's old emissive triangles (ordered-uint minima / maxima, one atomic per
 *     wavefront and word), the early-out of the pass below.
 *   k_light_follow<DIRECT>: one lane per record. Shaded records with M > 0 whose hit_p lies in that box, grown by what the exact test
 *     admits around a triangle (eps_tri off its plane, LF_TAU_B x an edge within it: no accepted point lies outside), locate their
 *     triangle and are carried to its new vertices (the caller's span, staged on the device before the old tables are overwritten)
 *     in the same launch; everything else keeps its bytes and walks nothing.
 *       DIRECT: a loop over the span's old light ids (small spans; the host selects it by the light count).
 *       else: a POINT QUERY on the old wide tree: a stack walk over the 48-byte records (bvh.h) that descends into a child iff hit_p
 *         lies in the child's box, decoded as every walk decodes it (origin + q * scale), grown by eps_box = LF_TAU_P x the largest
 *         |coordinate| of the root box, and runs lf_locate_test on the leaves whose triangle index lies in the span. The boxes are
 *         conservative and eps_tri <= eps_box, so the accepted set is that of a loop over the span (tests/test_gpu_light_follow.py
 *         holds it to that bit for bit). Pre-split fragments put a triangle into several leaves: the minimum is idempotent. The
 *         stack is trace_wide's: WIDE_LDS_STACK rows in LDS, the rest in scratch, at most 3 pushes per level (height checked at
 *         build). Leaves are tested where they are met: a point meets a handful, there is nothing to batch.
 * Counters (examined, located, moved, emptied): summed per workgroup in LDS, then one atomic per non-zero sum into one of 64 slots.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "bvh.h"
#include "bvh_build_device.h" /* sah_enc / sah_dec */
#include "light_follow.h"

namespace rt
{

/* spans of at most this many old lights take the direct loop (rt_temporal_light_motion_path overrides it for tests and measurements).
 * Measured at 2 lights only (1080p, three buffers: 0.107 ms of launches against the point query's 0.224); where the paths cross was not */
constexpr int LF_DIRECT_MAX_DEFAULT = 16;

struct LightFollowParams
{
    uint32_t n_records;
    uint32_t first, count;          /* the updated span */
    const float* tris_old;          /* all triangles, 15 floats each, before the update */
    const float* tris_new;          /* the span's new triangles, 15 floats each */
    const uint32_t* ids;            /* DIRECT: the span's old emissive triangles */
    uint32_t n_ids;
    const float4* wide;             /* the old tree */
    uint32_t n_wide;
    const unsigned int* box;        /* k_light_follow_box's six words */
    unsigned long long* counters;   /* [LF_COUNTER_WORDS] */
};

/* box[0..2] start as 0xffffffff, box[3..5] as 0 */
__global__ void k_light_follow_box(const float* __restrict__ tris, uint32_t first, uint32_t count, unsigned int* __restrict__ box)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int k[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (i < count)
    {
        const float* t = tris + 15 * (size_t)(first + i);
        if (lf_emissive(F3(t[12], t[13], t[14])))
            for (int a = 0; a < 3; ++a)
            {
                /* NaN coordinates drop out of fminf / fmaxf; a triangle of NaNs only leaves the box as it was */
                const float lo = fminf(fminf(t[a], t[3 + a]), t[6 + a]), hi = fmaxf(fmaxf(t[a], t[3 + a]), t[6 + a]);
                if (lo == lo) k[a] = sah_enc(lo);
                if (hi == hi) k[3 + a] = sah_enc(hi);
            }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a)
        {
            k[a] = min(k[a], (unsigned int)__shfl_xor((int)k[a], off, 64));
            k[3 + a] = max(k[3 + a], (unsigned int)__shfl_xor((int)k[3 + a], off, 64));
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 3; ++a)
        {
            if (k[a] != 0xffffffffu) atomicMin(&box[a], k[a]);
            if (k[3 + a] != 0u) atomicMax(&box[3 + a], k[3 + a]);
        }
}

/* counters: LF_COUNTER_SLOTS slots of 4 x 64 bit, summed by the reader. A workgroup adds its four sums to slot blockIdx % SLOTS, and
 * only those that are not 0: one address saw an atomic per wavefront and counter before (32 000 per launch at 1080p) */
constexpr int LF_COUNTER_SLOTS = 64;
constexpr int LF_COUNTER_WORDS = 4 * LF_COUNTER_SLOTS;
RT_DEV void lf_count(unsigned int* __restrict__ s_count, bool mine)
{
    const unsigned long long b = __ballot(mine); /* called where the wavefront has converged: lane 0 is there */
    if (b != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(s_count, (unsigned int)__popcll(b));
}

template <bool DIRECT>
__global__ void __launch_bounds__(BLOCK_THREADS) k_light_follow(const LightFollowParams P, float4* __restrict__ rec, float4* __restrict__ radb)
{
    __shared__ uint32_t s_stack[DIRECT ? 1 : WIDE_LDS_STACK * BLOCK_THREADS];
    __shared__ unsigned int s_count[4];
    if (threadIdx.x < 4u) s_count[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    bool examined = false, inside = false;
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0, rq = q0;
    if (i < P.n_records)
    {
        q1 = rec[4 * (size_t)i + 1];
        const uint32_t mb = as_uint(q1.w);
        examined = (mb & RES_SHADED_BIT) != 0u && (mb & RES_M_MASK) != 0u;
    }
    if (examined)
    {
        q0 = rec[4 * (size_t)i];
        /* the box of the span's old lights, grown by what lf_locate_test admits around a triangle: the largest eps_tri among them off
         * the plane, and LF_TAU_B x an edge within it (an edge is at most the box's extents added up). An empty box (no finite light)
         * admits nothing */
        const f3 blo = F3(sah_dec(P.box[0]), sah_dec(P.box[1]), sah_dec(P.box[2])), bhi = F3(sah_dec(P.box[3]), sah_dec(P.box[4]), sah_dec(P.box[5]));
        const float eps = lf_eps_box(blo, bhi) + 2.0f * LF_TAU_B * ((bhi.x - blo.x) + (bhi.y - blo.y) + (bhi.z - blo.z));
        inside = q0.x >= blo.x - eps && q0.x <= bhi.x + eps && q0.y >= blo.y - eps && q0.y <= bhi.y + eps && q0.z >= blo.z - eps && q0.z <= bhi.z + eps;
    }
    LfMatch best;
    best.ok = false; best.dist = 0.0f; best.u = 0.0f; best.v = 0.0f; best.area2 = 0.0f;
    int best_t = -1;
    if (inside)
    {
        rq = radb[i];
        const f3 hit_p = F3(q0.x, q0.y, q0.z), hit_n = F3(q1.x, q1.y, q1.z), rad = F3(rq.x, rq.y, rq.z);
        auto test = [&](uint32_t t) {
            const float* o = P.tris_old + 15 * (size_t)t;
            const LfMatch m = lf_locate_test(hit_p, hit_n, rad, F3(o[0], o[1], o[2]), F3(o[3], o[4], o[5]), F3(o[6], o[7], o[8]), F3(o[12], o[13], o[14]));
            if (lf_better(m, (int)t, best, best_t)) { best = m; best_t = (int)t; }
        };
        if (DIRECT)
        {
            for (uint32_t j = 0; j < P.n_ids; ++j) test(P.ids[j]);
        }
        else if (P.n_wide > 0u)
        {
            uint32_t ovf[WIDE_OVF_STACK];
            int sp = 0;
            const int lane_slot = threadIdx.x;
            auto push = [&](uint32_t e) {
                if (sp < WIDE_LDS_STACK) s_stack[sp * BLOCK_THREADS + lane_slot] = e;
                else if (sp < RT_WIDE_TOTAL_STACK) ovf[sp - WIDE_LDS_STACK] = e;
                if (sp < RT_WIDE_TOTAL_STACK) ++sp; /* never reached: 3 pushes per level, height checked at build */
            };
            auto pop = [&]() -> uint32_t {
                --sp;
                return sp < WIDE_LDS_STACK ? s_stack[sp * BLOCK_THREADS + lane_slot] : ovf[sp - WIDE_LDS_STACK];
            };
            constexpr uint32_t NONE = 0x7fffffffu;
            float eps_box = 0.0f;
            uint32_t cur = 0u; /* the root is always an inner record */
            bool at_root = true;
            while (cur != NONE)
            {
                const uint32_t r = cur & ~WIDE_LEAF_BIT;
                if (r >= P.n_wide) break; /* never: children lie inside the array */
                const float4* g = P.wide + WIDE_STRIDE * (size_t)r;
                if (cur & WIDE_LEAF_BIT)
                {
                    const uint32_t t = as_uint(g[2].y);
                    if (t - P.first < P.count) test(t);
                    cur = sp ? pop() : NONE;
                    continue;
                }
                const float4 a0 = g[0], a1 = g[1], a2 = g[2];
                const uint32_t e = as_uint(a0.w), base = as_uint(a1.x), meta = as_uint(a1.y);
                const uint32_t lx = as_uint(a1.z), ly = as_uint(a1.w), lz = as_uint(a2.x), hx = as_uint(a2.y), hy = as_uint(a2.z), hz = as_uint(a2.w);
                const float sx = wide_scale(e, 0), sy = wide_scale(e, 1), sz = wide_scale(e, 2);
                f3 clo[4], chi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    clo[k] = F3(a0.x + wide_byte(lx, k) * sx, a0.y + wide_byte(ly, k) * sy, a0.z + wide_byte(lz, k) * sz);
                    chi[k] = F3(a0.x + wide_byte(hx, k) * sx, a0.y + wide_byte(hy, k) * sy, a0.z + wide_byte(hz, k) * sz);
                }
                if (at_root)
                {
                    /* the root box: the union of record 0's children */
                    f3 rlo = F3(INFINITY, INFINITY, INFINITY), rhi = F3(-INFINITY, -INFINITY, -INFINITY);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((meta >> (8 * k)) & 0xffu)
                        {
                            rlo = F3(fminf(rlo.x, clo[k].x), fminf(rlo.y, clo[k].y), fminf(rlo.z, clo[k].z));
                            rhi = F3(fmaxf(rhi.x, chi[k].x), fmaxf(rhi.y, chi[k].y), fmaxf(rhi.z, chi[k].z));
                        }
                    eps_box = lf_eps_box(rlo, rhi);
                    at_root = false;
                }
                uint32_t next = NONE;
#pragma unroll
                for (int k = 3; k >= 0; --k)
                {
                    const uint32_t m = (meta >> (8 * k)) & 0xffu;
                    const bool in = m != 0u && hit_p.x >= clo[k].x - eps_box && hit_p.x <= chi[k].x + eps_box && hit_p.y >= clo[k].y - eps_box &&
                                    hit_p.y <= chi[k].y + eps_box && hit_p.z >= clo[k].z - eps_box && hit_p.z <= chi[k].z + eps_box;
                    if (in)
                    {
                        if (next != NONE) push(next);
                        next = (base + (uint32_t)k) | (m == 2u ? WIDE_LEAF_BIT : 0u);
                    }
                }
                cur = next != NONE ? next : (sp ? pop() : NONE);
            }
        }
    }
    bool moved = false, emptied = false;
    if (best_t >= 0)
    {
        const float* o = P.tris_old + 15 * (size_t)best_t;
        const float* n = P.tris_new + 15 * (size_t)((uint32_t)best_t - P.first);
        float ob[15], nb[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) { ob[k] = o[k]; nb[k] = n[k]; }
        LfSample s;
        s.hit_p = F3(q0.x, q0.y, q0.z); s.hit_n = F3(q1.x, q1.y, q1.z); s.rad = F3(rq.x, rq.y, rq.z);
        s.ucw = q0.w; s.lum = 0.0f;
        const LfOutcome out = lf_apply(s, best, ob, nb);
        if (out == LF_MOVED)
        {
            moved = true;
            float4* R = rec + 4 * (size_t)i;
            R[0] = make_float4(s.hit_p.x, s.hit_p.y, s.hit_p.z, s.ucw);
            R[1] = make_float4(s.hit_n.x, s.hit_n.y, s.hit_n.z, q1.w);
            reinterpret_cast<float*>(R + 2)[3] = s.lum;
            radb[i] = make_float4(s.rad.x, s.rad.y, s.rad.z, 0.0f);
        }
        else if (out == LF_EMPTIED)
        {
            emptied = true;
            float4* R = rec + 4 * (size_t)i;
            const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            R[0] = z;
            R[1] = make_float4(0.0f, 0.0f, 0.0f, as_float(RES_SHADED_BIT));
            R[2] = z;
            R[3] = z;
            radb[i] = z;
        }
    }
    lf_count(s_count + 0, examined);
    lf_count(s_count + 1, best_t >= 0);
    lf_count(s_count + 2, moved);
    lf_count(s_count + 3, emptied);
    __syncthreads(); /* every thread of the workgroup arrives: nothing above returns */
    if (threadIdx.x < 4u && s_count[threadIdx.x] != 0u)
        atomicAdd(P.counters + 4 * (blockIdx.x % LF_COUNTER_SLOTS) + threadIdx.x, (unsigned long long)s_count[threadIdx.x]);
}

}  // namespace rt
