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
 *     (wide_quant_scale / wide_quant_child).
 *   fragments (once per scene, at its first update, while the build's triangles are still in place): the build cut large
 *     triangles into box fragments, one leaf each. The split is run again with barycentric coordinates carried along
 *     (bvh_fragment.h: same positions, same fragments, same order) and every fragment's polygon, at most 12 (u, v) pairs, is
 *     kept in a table. The build left "1 + fragment number within the triangle" in word 10 of such a leaf (0 elsewhere; no
 *     walk uses the word); k_frag_assign turns it into 1 + a table slot. Slots are numbered in the order the refit visits
 *     the leaves (level list position, then child), and the table is vertex-major — pair i of slot s at uv[i * F + s] — so
 *     the lanes of a wavefront, which hold consecutive list positions, read consecutive addresses. 97 bytes per fragment
 *     (12 pairs + a count byte), fragments of split triangles only.
 *     A leaf with a slot gets the box of its polygon under the NEW vertices (frag_box) instead of the whole triangle's:
 *     bvh_fragment.h has the argument that the padded boxes of a triangle's fragments still cover every point of it, seams
 *     and T-junctions included, whatever the new vertices are. They derive from the build's (u, v) at every update: no drift.
 *     Without a table (builders 0-2 of the experiments library, no pre-split, nothing split) every leaf of a triangle gets
 *     the whole triangle's box, as before: conservative, so the walks stay exact (boxes only prune), only slower.
 *   cost (rt_bvh_cost): k_bvh_cost sums, over the listed inner records, the half-areas of the child boxes as a walk
 *     decodes them.
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
                              const unsigned int* __restrict__ bounds, float* __restrict__ boxes, uint32_t* __restrict__ recs,
                              const float* __restrict__ frag_uv /* vertex-major, or nullptr */, const uint8_t* __restrict__ frag_n, uint32_t n_frags)
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
            const uint32_t slot1 = frag_uv ? L[10] : 0u;
            /* fewer than 3 vertices: a slot the table never filled. The whole triangle's box then, never an empty one */
            const int fn = (slot1 != 0u && slot1 <= n_frags) ? (int)frag_n[slot1 - 1u] : 0;
            if (fn >= 3 && fn <= FRAG_MAX_VERTS)
            {
                /* a fragment of a split triangle: the box of its polygon under the new vertices */
                const uint32_t slot = slot1 - 1u;
                float flo[3], fhi[3];
                frag_box(t, t + 3, t + 6, frag_uv + 2 * (size_t)slot, fn, 2 * (size_t)n_frags, flo, fhi);
                for (int a = 0; a < 3; ++a) { clo[k][a] = flo[a] - pad; chi[k][a] = fhi[a] + pad; }
            }
            else
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

/* ------------------------------------------------------------------ the fragment table (once per scene) */
/* fc[i] = fragments of triangle i if it was split, else 0 */
__global__ void k_frag_counts(int n, const uint32_t* __restrict__ counts, uint32_t* __restrict__ fc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fc[i] = counts[i] > 1u ? counts[i] : 0u;
}
/* list position p -> leaf children that are fragments (word 10 != 0) */
__global__ void k_frag_leaves(const uint32_t* __restrict__ list, uint32_t n, const uint32_t* __restrict__ recs, uint32_t* __restrict__ per_rec)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t* R = recs + 4 * WIDE_STRIDE * (size_t)list[p];
    const uint32_t base = R[4], meta = R[5];
    uint32_t m = 0;
    for (int k = 0; k < 4; ++k)
        if (((meta >> (8 * k)) & 0xffu) == 2u && recs[4 * WIDE_STRIDE * (size_t)(base + (uint32_t)k) + 10] != 0u) ++m;
    per_rec[p] = m;
}
/* slots in visiting order: word 10 of a fragment leaf becomes 1 + slot, slot_of[frag_off[triangle] + fragment] = slot. A leaf
 * whose fragment number or slot is out of range (none, unless the records are not this build's) gets 0: whole-triangle box. */
__global__ void k_frag_assign(const uint32_t* __restrict__ list, uint32_t n, uint32_t* __restrict__ recs, const uint32_t* __restrict__ slot_base,
                              const uint32_t* __restrict__ counts, const uint32_t* __restrict__ frag_off, uint32_t n_frags, int n_tris,
                              uint32_t* __restrict__ slot_of)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t* R = recs + 4 * WIDE_STRIDE * (size_t)list[p];
    const uint32_t base = R[4], meta = R[5];
    uint32_t slot = slot_base[p];
    for (int k = 0; k < 4; ++k)
    {
        if (((meta >> (8 * k)) & 0xffu) != 2u) continue;
        uint32_t* L = recs + 4 * WIDE_STRIDE * (size_t)(base + (uint32_t)k);
        const uint32_t j1 = L[10];
        if (j1 == 0u) continue;
        const uint32_t t = L[9];
        if (t < (uint32_t)n_tris && counts[t] > 1u && j1 <= counts[t] && slot < n_frags)
        {
            slot_of[frag_off[t] + j1 - 1u] = slot;
            L[10] = slot + 1u;
        }
        else
            L[10] = 0u; /* whole-triangle box */
        ++slot;
    }
}
/* the split again, with (u, v): polygon j of split triangle i -> slot slot_of[frag_off[i] + j] of the vertex-major table */
__global__ void k_frag_emit(const float* __restrict__ tris, int n, float L, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ frag_off,
                            const uint32_t* __restrict__ slot_of, uint32_t n_frags, float* __restrict__ frag_uv, uint8_t* __restrict__ frag_n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = counts[i];
    if (cnt <= 1u) return;
    const uint32_t off = frag_off[i];
    frag_split<true>(tris + 15 * (size_t)i, L, [&](uint32_t j, const FragPoly<true>& q, const float*, const float*) {
        if (j >= cnt) return;
        const uint32_t slot = slot_of[off + j];
        if (slot >= n_frags) return;
        frag_n[slot] = (uint8_t)q.n;
        for (int v = 0; v < q.n; ++v)
        {
            float* o = frag_uv + 2 * ((size_t)v * n_frags + slot);
            o[0] = q.uv[v][0];
            o[1] = q.uv[v][1];
        }
    });
}

/* ------------------------------------------------------------------ rt_bvh_cost */
/* out[0] += half-areas of the occupied child slots of the listed inner records, decoded as the walks decode them
 * (lo + q * scale in binary32; q * scale is exact); out[1] = half-area of the root's box (the union of record 0's children) */
__global__ __launch_bounds__(256) void k_bvh_cost(const uint32_t* __restrict__ list, uint32_t n, const uint32_t* __restrict__ recs, double* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double sum = 0.0;
    if (i < n)
    {
        const uint32_t r = list[i];
        const uint32_t* R = recs + 4 * WIDE_STRIDE * (size_t)r;
        const uint32_t e = R[3], meta = R[5];
        float ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 4; ++k)
        {
            if (((meta >> (8 * k)) & 0xffu) == 0u) continue;
            double d[3];
            for (int a = 0; a < 3; ++a)
            {
                const float o = __uint_as_float(R[a]), sc = __uint_as_float(((e >> (8 * a)) & 0xffu) << 23);
                const float lo = o + wide_byte(R[6 + a], k) * sc, hi = o + wide_byte(R[9 + a], k) * sc;
                d[a] = (double)hi - (double)lo;
                ulo[a] = fminf(ulo[a], lo);
                uhi[a] = fmaxf(uhi[a], hi);
            }
            sum += d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
        }
        if (r == 0u)
        {
            const double dx = (double)uhi[0] - (double)ulo[0], dy = (double)uhi[1] - (double)ulo[1], dz = (double)uhi[2] - (double)ulo[2];
            out[1] = dx * dy + dy * dz + dz * dx;
        }
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    __shared__ double s_sum[4];
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) atomicAdd(&out[0], (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
}

}  // namespace rt
