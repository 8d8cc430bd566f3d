/*
 * bvh_fragment.h — the arithmetic of the build's early split clipping (bvh_build_device.h::k_split_refs) and of the boxes its
 * fragments get when rt_scene_update moves their triangle (bvh_refit.h::k_refit_level). RT_HD, so hipcc and
 * `g++ -ffp-contract=off` compile the same expressions (tests/test_bvh_fragment_cpu.py restates and checks them on the CPU).
 *
 * A fragment is a convex polygon of at most FRAG_MAX_VERTS vertices clipped out of its triangle by axis-aligned planes.
 * FragPoly<true> carries, beside each vertex position, its barycentric coordinates (u, v) in the SOURCE triangle
 * (P = (1 - u - v) A + u B + v C): the corners start as (0,0), (1,0), (0,1) and a cut vertex interpolates them with the same
 * `t` as its position. Positions come out of frag_clip by the expressions, in the order, of the clip the build has always
 * used, so FragPoly<false> and FragPoly<true> make the same boxes bit for bit; (u, v) ride along and decide nothing.
 *
 * COVERAGE after an update (why the refit may give leaf j the box of frag_box over ITS polygon only). Let T be the
 * parameter triangle {u, v >= 0, u + v <= 1}.
 *   1. A split cuts a polygon by a plane x_a = s on an axis where the polygon's extent exceeds L > 0, so x_a is a
 *      non-constant affine function of (u, v) — also for a triangle with repeated or collinear vertices — and "left" and
 *      "right" are the two closed sides of ONE line of the parameter plane. Both sides visit the same edges c -> d in the
 *      same direction and compute the same t, so the two cut vertices they share are the same bits: in exact arithmetic
 *      over the stored float (u, v), left and right tile the polygon whose boundary is the parent's with the two cut
 *      vertices inserted.
 *   2. A cut vertex is rounded: c + (d - c) * t in binary32 on coordinates in [0, 1] is three roundings of at most 2^-25
 *      each, so it lies within delta = 1.3e-7 of the edge c -> d (an error of t only moves it ALONG the edge, and both
 *      sides share it). What two children miss of their parent is therefore a sliver of width delta along the parent's
 *      edge; this is also what a T-junction is (the neighbour across that edge keeps c -> d uncut, or cuts it elsewhere).
 *      Slivers add up along a chain of D cuts, so every point of T is within D * delta (parameter units) of a point
 *      (u', v') of some emitted polygon. D is small: a cut sits on the grid line nearest the middle of the polygon's longest
 *      extent e (or in the middle), leaving at most e / 2 + L / 2, and cutting stops at e <= L, at FRAG_MAX_PER_TRI
 *      fragments or at a full stack: D <= 3 * (2 + log2(e / L)), about 40 for the 4096 fragments of a triangle.
 *   3. The map (u, v) -> (1 - u - v) A + u B + v C is affine for ANY new A, B, C (moved, rotated, scaled, mirrored,
 *      collapsed to a segment or a point): the image of (u', v') is a convex combination of the images of its polygon's
 *      vertices and lies in their exact box; a parameter error of e moves the image by at most e * (|B - A| + |C - A|)
 *      <= 4 e m per coordinate, m = the largest |coordinate| of the new triangle; and frag_point's binary32 evaluation
 *      (5 roundings of magnitudes <= 3 m) is within 1e-6 m of the exact image.
 *   So every point of the new triangle lies within (4 * D * 1.3e-7 + 1e-6) m of the box frag_box returns for one of its
 *   fragments: 2.2e-5 m at D = 40. The refit pads by 4e-5 * max(1, M), M >= m the largest |coordinate| of the scene.
 *   WHAT THE PAD IS FOR, and what is left of it: the pad exists because an accepted hit point lies within rounding
 *   distance of its triangle, not on it (restir_rt.hip, where the build computes it); the walk must not prune the box that
 *   holds that point. The build spends about 1e-7 m of it on its own rounded cut vertices. The refit's fragment error comes out
 *   of the same pad: in the worst case above it takes 55 % and leaves 1.8e-5 m — 300 units in the last place of m — for the
 *   hit point; a chain of more than 40 cuts would leave less, and from D = 75 nothing, which the caps on the split keep out
 *   of reach (4096 fragments, cuts that halve). The bound is a worst case in every term at once: tests/
 *   test_bvh_fragment_cpu.py measures that sampled points need less than 0.1 % of the pad, so in practice the hit point keeps
 *   all but a thousandth of what the build gives it. Every update evaluates the BUILD-time (u, v), never a previous update's
 *   boxes, so nothing drifts.
 *   (A polygon that would exceed FRAG_MAX_VERTS drops the surplus vertices, as the build's clip always has. A triangle cut
 *   by the six planes of a box has at most 9.)
 */
#pragma once
#include "rt_device.h"

namespace rt
{

constexpr int FRAG_MAX_VERTS = 12;
constexpr int FRAG_SPLIT_STACK = 20;        /* polygons a triangle's split recursion may have pending */
constexpr unsigned int FRAG_MAX_PER_TRI = 4096u;

template <bool UV>
struct FragParams
{
    float uv[FRAG_MAX_VERTS][2];
};
template <>
struct FragParams<false> /* the build's polygons: positions only, the size they have always had */
{
};
template <bool UV>
struct FragPoly : FragParams<UV>
{
    int n;
    float v[FRAG_MAX_VERTS][3];
};

template <bool UV>
RT_HD void frag_from_triangle(const float* t /* 9 floats */, FragPoly<UV>& p)
{
    p.n = 3;
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p.v[k][a] = t[3 * k + a];
    if constexpr (UV)
    {
        p.uv[0][0] = 0.0f; p.uv[0][1] = 0.0f;
        p.uv[1][0] = 1.0f; p.uv[1][1] = 0.0f;
        p.uv[2][0] = 0.0f; p.uv[2][1] = 1.0f;
    }
}

template <bool UV>
RT_HD void frag_bounds(const FragPoly<UV>& p, float* lo, float* hi)
{
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int i = 0; i < p.n; ++i)
        for (int a = 0; a < 3; ++a)
        {
            lo[a] = fminf(lo[a], p.v[i][a]);
            hi[a] = fmaxf(hi[a], p.v[i][a]);
        }
}

/* the side x_a <= s (sign < 0) or x_a >= s (sign > 0) of p; a cut vertex takes (u, v) by the t of its position */
template <bool UV>
RT_HD void frag_clip(const FragPoly<UV>& p, int a, float s, int sign, FragPoly<UV>& o)
{
    o.n = 0;
    for (int i = 0; i < p.n; ++i)
    {
        const int j = (i + 1) % p.n;
        const float* c = p.v[i];
        const float* d = p.v[j];
        const bool cin = sign > 0 ? c[a] >= s : c[a] <= s;
        const bool din = sign > 0 ? d[a] >= s : d[a] <= s;
        if (cin && o.n < FRAG_MAX_VERTS)
        {
            o.v[o.n][0] = c[0]; o.v[o.n][1] = c[1]; o.v[o.n][2] = c[2];
            if constexpr (UV) { o.uv[o.n][0] = p.uv[i][0]; o.uv[o.n][1] = p.uv[i][1]; }
            o.n++;
        }
        if (cin != din && o.n < FRAG_MAX_VERTS)
        {
            const float t = (s - c[a]) / (d[a] - c[a]);
            for (int k = 0; k < 3; ++k) o.v[o.n][k] = c[k] + (d[k] - c[k]) * t;
            o.v[o.n][a] = s;
            if constexpr (UV)
                for (int k = 0; k < 2; ++k) o.uv[o.n][k] = p.uv[i][k] + (p.uv[j][k] - p.uv[i][k]) * t;
            o.n++;
        }
    }
}

/* The split recursion of one triangle with a per-thread stack: large polygons are cut on the global L-grid (so that
 * fragments of neighbours line up) until their largest extent is at most L, the triangle has FRAG_MAX_PER_TRI fragments
 * or the stack is full. sink(j, polygon, lo, hi) receives fragment j = 0, 1, ... with its unpadded box; returns their number. */
template <bool UV, class Sink>
RT_HD unsigned int frag_split(const float* t /* 9 floats */, float L, Sink&& sink)
{
    FragPoly<UV> stack[FRAG_SPLIT_STACK];
    int sp = 1;
    frag_from_triangle<UV>(t, stack[0]);
    unsigned int emitted = 0;
    while (sp > 0)
    {
        const FragPoly<UV> q = stack[--sp];
        float lo[3], hi[3];
        frag_bounds(q, lo, hi);
        int a = 0;
        for (int k = 1; k < 3; ++k)
            if (hi[k] - lo[k] > hi[a] - lo[a]) a = k;
        const float ext = hi[a] - lo[a];
        bool split = L > 0.0f && ext > L && emitted + (unsigned int)sp < FRAG_MAX_PER_TRI && q.n >= 3 && sp + 2 <= FRAG_SPLIT_STACK;
        float s = 0.0f;
        if (split)
        {
            const float mid = 0.5f * (lo[a] + hi[a]);
            s = L * floorf(mid / L + 0.5f);
            if (!(s > lo[a] + 0.01f * ext && s < hi[a] - 0.01f * ext)) s = mid;
            if (!(s > lo[a] && s < hi[a])) split = false;
        }
        if (split)
        {
            FragPoly<UV> l, r;
            frag_clip(q, a, s, -1, l);
            frag_clip(q, a, s, +1, r);
            if (l.n >= 3 && r.n >= 3)
            {
                stack[sp++] = l;
                stack[sp++] = r;
                continue;
            }
        }
        sink(emitted, q, lo, hi);
        ++emitted;
    }
    return emitted;
}

/* The fragment length both builders use (host code; the ONE owner of the search). budget = 4 * triangles + 1024 references.
 * count(L) returns the scene's total number of fragments at length L as uint64_t — a triangle gives up to FRAG_MAX_PER_TRI, so
 * above 2^20 triangles a 32-bit total can wrap and pass the test below: the callers sum in 64 bits (the device build by a
 * 64-bit reduction over the per-triangle counts, the host path by the size of its vector).
 *   - L0 is returned unchanged when it fits (or is <= 0: no splitting, one reference per triangle).
 *   - Up to FRAG_FIT_ROUNDS steps of 1.5 x, as the build has always relaxed L: a scene that fitted within them keeps its L bit
 *     for bit.
 *   - After that L doubles until the count fits. It ends: frag_split cuts a polygon only while its extent exceeds L, so from
 *     L >= the largest triangle extent (at the latest L = +inf, which binary32 doubling reaches in under 280 steps from any
 *     L > 0) every triangle is one fragment, and triangles <= budget.
 * The LAST call of count is at the returned L, so what count left behind (per-triangle counts, the fragments themselves)
 * belongs to it; *total, if given, receives that count. tests/test_bvh_presplit_budget_cpu.py runs it, beside the loop it
 * replaced, on scenes that loop left far over the budget. */
constexpr int FRAG_FIT_ROUNDS = 16;
template <class Count>
inline float frag_fit_length(float L0, uint64_t budget, Count&& count, uint64_t* total = nullptr)
{
    float L = L0;
    for (int it = 0;; ++it)
    {
        const uint64_t n = count(L);
        if (n <= budget || !(L > 0.0f))
        {
            if (total) *total = n;
            return L;
        }
        L *= it < FRAG_FIT_ROUNDS - 1 ? 1.5f : 2.0f;
    }
}

/* (1 - u - v) A + u B + v C: a corner's (u, v) gives its vertex back exactly */
RT_HD void frag_point(const float* A, const float* B, const float* C, float u, float v, float* p)
{
    const float w = 1.0f - u - v;
    for (int a = 0; a < 3; ++a) p[a] = w * A[a] + u * B[a] + v * C[a];
}

/* box of fragment `uv` (n pairs, `stride` floats apart: the refit's table is vertex-major) under the vertices A, B, C */
RT_HD void frag_box(const float* A, const float* B, const float* C, const float* uv, int n, size_t stride, float* lo, float* hi)
{
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int i = 0; i < n; ++i)
    {
        float p[3];
        frag_point(A, B, C, uv[(size_t)i * stride], uv[(size_t)i * stride + 1], p);
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
    }
}

}  // namespace rt
