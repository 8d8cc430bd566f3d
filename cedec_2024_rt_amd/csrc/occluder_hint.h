/*
 * occluder_hint.h — the per-pixel record of triangles that occluded the pixel's earlier candidate shadow rays
 * (k_generate_candidate, frame_kernels.h). RT_HD, so hipcc and a plain g++ compile the same functions:
 * tests/test_occluder_hint_cpu.py runs them on the host against a model of the rules below.
 *
 * A record holds N triangle indices, most recently used first; an entry that names no triangle of the scene (-1 = empty,
 * or anything at or above the triangle count) is never tested. WHY ANY CONTENT IS SAFE: a hint is only ever used for one
 * exact intersect_ray_triangle of that triangle's current vertices with the ray's own origin, direction and range. A hit
 * means brute force over all triangles hits, which is what the any-hit walk answers (tests/test_gpu_targeted_rays.py); a
 * miss leaves the walk to run. So the record needs no epoch, may be written by racing lanes, and may differ from run to
 * run: the images may not.
 *
 *   test order       positions 0, 1, ..., N-1, skipping entries that name no triangle (hint_pending)
 *   hit at k > 0     entry k moves to the front, entries 0 .. k-1 move down one (hint_hit); k = 0 changes nothing
 *   new occluder     the walk named a triangle: it goes to the front and the last entry is dropped; if the record holds it
 *                    already it moves to the front instead, so that there are no duplicates (hint_insert)
 * Both updates return whether the record changed: a lane whose record did not change writes nothing.
 */
#pragma once
#include "rt_device.h"

namespace rt
{

/* remembered triangles per pixel: 1, 2 and 4 were measured (docs/MEASUREMENT_LOG_r19.md) */
#ifndef RT_OCCLUDER_HINTS
#define RT_OCCLUDER_HINTS 4
#endif
constexpr int OCCLUDER_HINTS = RT_OCCLUDER_HINTS;
static_assert(OCCLUDER_HINTS == 1 || OCCLUDER_HINTS == 2 || OCCLUDER_HINTS == 4, "a record is one 4-, 8- or 16-byte word");

template <int N>
struct OccluderHints
{
    int tri[N];
};

template <int N>
RT_HD OccluderHints<N> hint_empty()
{
    OccluderHints<N> h;
    for (int k = 0; k < N; ++k) h.tri[k] = -1;
    return h;
}

/* entry k names a triangle of a scene of n_tris triangles: the only entries that are tested */
template <int N>
RT_HD bool hint_pending(const OccluderHints<N>& h, int k, int n_tris)
{
    return (uint32_t)h.tri[k] < (uint32_t)n_tris;
}

/* the triangle at position k occluded the ray */
template <int N>
RT_HD bool hint_hit(OccluderHints<N>& h, int k)
{
    if (k <= 0) return false;
    const int t = h.tri[k];
    for (int j = N - 1; j > 0; --j)
        if (j <= k) h.tri[j] = h.tri[j - 1];
    h.tri[0] = t;
    return true;
}

/* the walk found `tri` occluding the ray */
template <int N>
RT_HD bool hint_insert(OccluderHints<N>& h, int tri)
{
    if (tri < 0 || h.tri[0] == tri) return false;
    int k = N - 1; /* the entry that leaves its place: the one that holds tri already, else the last */
    for (int j = N - 1; j > 0; --j)
        if (h.tri[j] == tri) k = j;
    for (int j = N - 1; j > 0; --j)
        if (j <= k) h.tri[j] = h.tri[j - 1];
    h.tri[0] = tri;
    return true;
}

} // namespace rt
