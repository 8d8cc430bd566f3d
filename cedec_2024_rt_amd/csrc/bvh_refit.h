/*
 * bvh_refit.h — refit of the 4-wide quantised tree (bvh.h) after rt_scene_update moved triangles: the counterpart of HIPRT's
 * hiprtBuildOperationUpdate. Topology stays as the build left it (record count, child order, base / meta words, height, so the
 * traversal stack bound holds); only the boxes change.
 *
 *   topology (once per scene, at its first update): a top-down pass over the records themselves — children sit at
 *     `base + k`, meta byte k says inner (1) or leaf (2) — lists the inner records level by level (k_refit_topo). Nothing
 *     depends on the order in which a builder allocated records, so every builder's tree (host or device collapse,
 *     breadth-first prefix of any length) refits the same way.
 *   refit (every update): one launch per level, deepest first (k_refit_level). An inner record rewrites its leaf
 *     children from the new triangles (9 floats + the unchanged index), takes its inner children's exact float boxes from
 *     the scratch array the level below wrote, stores its own box there and re-quantises with the build's quantiser
 *     (wide_quant_scale / wide_quant_child). A pre-split triangle's leaves each get the WHOLE triangle's box: conservative,
 *     so the walks stay exact (only prune), though they may visit more records than after a rebuild.
 * Leaf boxes carry the build's pad, 4e-5 * max(1, largest |coordinate|), over bounds that only grow: the whole scene at the
 * first update, then the union with each updated span (k_refit_bounds over the span). A larger pad only loosens boxes.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "bvh.h"
#include "bvh_build_device.h"

namespace rt
{

constexpr int REFIT_MAX_LEVELS = RT_WIDE_TOTAL_STACK; /* > the deepest tree the traversal stack admits ((64 - 1) / 3 + 1 levels) */

/* off[level + 2] starts where the list of level + 1 ends: k_refit_topo of `level` appends behind it */
__global__ void k_refit_topo_next(int level, uint32_t* __restrict__ off) { off[level + 2] = off[level + 1]; }

/* inner records of `level` (list[off[level] .. off[level + 1])) -> their inner children, appended to the list of level + 1 */
__global__ void k_refit_topo(int level, uint32_t* __restrict__ off, uint32_t* __restrict__ list, uint32_t cap, const uint32_t* __restrict__ recs)
{
    const uint32_t b = off[level], e = off[level + 1];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= e - b) return;
    const uint32_t* R = recs + 4 * WIDE_STRIDE * (size_t)list[b + t];
    const uint32_t base = R[4], meta = R[5];
    for (int k = 0; k < 4; ++k)
        if (((meta >> (8 * k)) & 0xffu) == 1u)
        {
            const uint32_t slot = atomicAdd(&off[level + 2], 1u);
            if (slot < cap) list[slot] = base + (uint32_t)k;
        }
}

/* scene bounds for the pad, in the ordered-uint encoding of k_tri_extents, grown to contain triangles [0, n) of `tris`: the
 * workgroup (256 threads) reduces its triangles first, so the six words see one atomic per workgroup instead of one per triangle */
__global__ void k_refit_bounds(const float* __restrict__ tris, int n, unsigned int* __restrict__ bounds)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int k[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (i < n)
    {
        const float* t = tris + 15 * (size_t)i;
        for (int a = 0; a < 3; ++a)
        {
            const float lo = fminf(fminf(t[a], t[3 + a]), t[6 + a]), hi = fmaxf(fmaxf(t[a], t[3 + a]), t[6 + a]);
            k[a] = sah_enc(lo);
            k[3 + a] = sah_enc(hi);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a)
        {
            k[a] = min(k[a], (unsigned int)__shfl_xor((int)k[a], off, 64));
            k[3 + a] = max(k[3 + a], (unsigned int)__shfl_xor((int)k[3 + a], off, 64));
        }
    __shared__ unsigned int s_k[4][6]; /* 256 threads = 4 wavefronts */
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 6; ++a) s_k[wave][a] = k[a];
    __syncthreads();
    if (threadIdx.x < 6u)
    {
        const int a = (int)threadIdx.x;
        unsigned int v = s_k[0][a];
        for (int w = 1; w < 4; ++w) v = a < 3 ? min(v, s_k[w][a]) : max(v, s_k[w][a]);
        if (a < 3) atomicMin(&bounds[a], v);
        else atomicMax(&bounds[a], v);
    }
}

/* the pad from the scene bounds */
RT_DEV float refit_pad(const unsigned int* __restrict__ bounds)
{
    float ext = 0.0f;
    for (int a = 0; a < 6; ++a) ext = fmaxf(ext, fabsf(sah_dec(bounds[a])));
    return 4e-5f * (ext > 1.0f ? ext : 1.0f);
}

/* one level of inner records, bottom-up: leaf children from the triangles, inner children from `boxes` (6 floats per record) */
__global__ void k_refit_level(const uint32_t* __restrict__ list, uint32_t n, const float* __restrict__ tris /* 15 floats each */,
                              const unsigned int* __restrict__ bounds, float* __restrict__ boxes, uint32_t* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = list[i];
    uint32_t* R = recs + 4 * WIDE_STRIDE * (size_t)r;
    const uint32_t base = R[4], meta = R[5];
    const float pad = refit_pad(bounds);
    float clo[4][3], chi[4][3];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 4; ++k)
    {
        const uint32_t type = (meta >> (8 * k)) & 0xffu;
        if (type == 0u) continue;
        if (type == 2u)
        {
            uint32_t* L = recs + 4 * WIDE_STRIDE * (size_t)(base + (uint32_t)k);
            const float* t = tris + 15 * (size_t)L[9];
            for (int a = 0; a < 3; ++a)
            {
                const float v0 = t[a], v1 = t[3 + a], v2 = t[6 + a];
                clo[k][a] = fminf(fminf(v0, v1), v2) - pad;
                chi[k][a] = fmaxf(fmaxf(v0, v1), v2) + pad;
            }
            for (int w = 0; w < 9; ++w) L[w] = __float_as_uint(t[w]);
        }
        else
        {
            const float* b = boxes + 6 * (size_t)(base + (uint32_t)k);
            for (int a = 0; a < 3; ++a) { clo[k][a] = b[a]; chi[k][a] = b[3 + a]; }
        }
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], clo[k][a]); hi[a] = fmaxf(hi[a], chi[k][a]); }
    }
    float* B = boxes + 6 * (size_t)r;
    for (int a = 0; a < 3; ++a) { B[a] = lo[a]; B[3 + a] = hi[a]; }
    float scale[3];
    const uint32_t ebits = wide_quant_scale(lo, hi, scale);
    uint32_t q[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
        if ((meta >> (8 * k)) & 0xffu) wide_quant_child(lo, scale, clo[k], chi[k], k, q);
    R[0] = __float_as_uint(lo[0]); R[1] = __float_as_uint(lo[1]); R[2] = __float_as_uint(lo[2]);
    R[3] = ebits;
    R[6] = q[0]; R[7] = q[1]; R[8] = q[2]; R[9] = q[3]; R[10] = q[4]; R[11] = q[5];
}

}  // namespace rt
