/*
 * light_grid.h — distance-aware light selection for the ReSTIR candidates (rt_light_grid): a two-level choice with
 * an exact pdf. The lights are grouped into spatial clusters ("runs"); a uniform grid of cells over the scene's bounding box holds, per
 * cell, an alias table over the runs, weighted by run power over squared distance; each run holds an alias table over its own lights,
 * weighted by area x luminance. A candidate finds the cell of its surface point, draws a run from the cell's table and a light from
 * the run's table. Every light belongs to exactly one run, so the path to a light is unique and its probability is the product of the
 * two probabilities the tables realise (light_alias.h: realised counts, never w / sum w). The kernel (frame_kernels.h,
 * k_generate_candidate<.., GRID>), the library's host code and the CPU restatement (tests/light_grid_ref.py) share this header.
 * Plain C++, binary32 in the order written unless a line says binary64; RT_HD where the device needs it.
 *
 * Bounds. lo / hi = componentwise min / max over every finite vertex coordinate of the scene's triangles (all zero if there is none).
 * Per axis, with N cells: size = (hi - lo) / N and inv = N / (hi - lo); an axis with hi == lo gets size = 1 and inv = 1.
 *     cell_of(p): per axis t = (p - lo) * inv, c = N - 1 if t >= N, (int)t if t > 0, else 0        index (cz N + cy) N + cx
 * which is min(max((int)t, 0), N - 1) wherever the conversion is defined, and defined everywhere else (NaN: 0): points outside clamp.
 * Cell c has the centre x_c = lo + ((float)c + 0.5f) * size per axis and the half diagonal h = 0.5f * length(size).
 *
 * Runs. B' = min(clusters, L). A light's centroid is ((v0 + v1) + v2) * (1.0f / 3.0f); the lights' own box llo / lhi is the box of
 * the lights' finite vertex coordinates, and a centroid is quantised per axis to 10 bits by cell_of's rule with N = 1024 over that box.
 * The lights are sorted by the 30-bit Morton code of the three (x in the lowest bit), ties by light index; perm[pos] is the light at
 * sorted position pos. Run r holds the positions [floor(r L / B'), floor((r + 1) L / B')): never empty. The light list and its index
 * order do not change. Inside a run, alias_build over light_weight of its lights in position order gives slots {thr, alias} (alias =
 * a slot of the same run) and realised counts K_i out of n_r 2^23. P_r = the binary64 sum, in position order, of the run's positive
 * finite weights. c_r = 0.5f * (lo_r + hi_r) of the run's finite vertex coordinates (zero if none), rho_r = the largest
 * length(v - c_r) over the run's vertices whose three coordinates are finite.
 *
 * Cell tables. w_{c,r} = (float)(P_r / max(|x_c - c_r|^2, (h + rho_r)^2)), the differences, squares, sums and the quotient in binary64
 * from the binary32 values above; a run with P_r = 0 has weight 0; any other weight is kept inside [FLT_MIN, FLT_MAX], so that it is
 * positive and finite: every run with a selectable light is selectable from every cell, which is what unbiasedness needs. The
 * denominator is the squared distance to the run's centre, but never less than the square of (cell half diagonal + run radius): a
 * point of the cell is at most that far from a light of a run whose centre lies inside the cell, so near runs are weighted alike and
 * no weight blows up. alias_build over the B' weights of a cell gives K_{c,r} out of B' 2^23.
 *
 * A candidate draws rv0, ra, rc, rb, bx, by, u in this order:
 *     s = light_slot(B', rv0)       r = light_select_slot(cell[c][s], s, ra)
 *     t = light_slot(n_r, rc)       pos = start_r + light_select_slot(run[start_r + t], t, rb)         light i = perm[pos]
 *     pdf_i = grid_pdf(light_select_prob(K_{c,r}, B'), light_select_prob(K_i, n_r) * 1.0f / area_i)     (the product of the two)
 * The second factor is what k_light_table stores in the light record; the device's light table of this mode is in position order,
 * so the kernel never needs perm.
 */
#pragma once
#include <stdint.h>

#include "light_alias.h"
#include "rt_device.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace rt
{

constexpr int kGridMaxCells = 32;      /* cells per axis */
constexpr int kGridMaxClusters = 256;
constexpr float kGridFltMin = 1.17549435e-38f;

struct GridBounds
{
    f3 lo, inv;
    int N;
};
struct GridRun
{
    uint32_t start, n; /* sorted positions [start, start + n) */
};
/* what a candidate reads */
struct GridView
{
    GridBounds b;
    uint32_t B;                 /* B' */
    const AliasSlot* cells;     /* N^3 x B' */
    const float* cell_prob;     /* N^3 x B': light_select_prob(K_{c,r}, B') */
    const GridRun* runs;        /* B' */
    const AliasSlot* run_slots; /* L, position order; alias = a slot of the same run */
};

RT_HD int grid_axis_cell(float p, float lo, float inv, int N)
{
    const float t = (p - lo) * inv;
    return t >= (float)N ? N - 1 : (t > 0.0f ? (int)t : 0);
}
RT_HD uint32_t grid_cell_of(const GridBounds& g, f3 p)
{
    const int cx = grid_axis_cell(p.x, g.lo.x, g.inv.x, g.N), cy = grid_axis_cell(p.y, g.lo.y, g.inv.y, g.N), cz = grid_axis_cell(p.z, g.lo.z, g.inv.z, g.N);
    return (uint32_t)((cz * g.N + cy) * g.N + cx);
}
/* the pdf of a light: the cell's factor times the record's (run factor * 1.0f / area), in this order */
RT_HD float grid_pdf(float cell_prob, float rec_pdf) { return cell_prob * rec_pdf; }
/* run and sorted position of a candidate; the cell's factor of its pdf comes back through cell_prob */
RT_HD uint32_t grid_select(const GridView& g, uint32_t cell, float rv0, float ra, float rc, float rb, float& cell_prob)
{
    const uint32_t base = cell * g.B;
    const uint32_t s = light_slot(g.B, rv0);
    const uint32_t r = light_select_slot(g.cells[base + s], s, ra);
    cell_prob = g.cell_prob[base + r];
    const GridRun run = g.runs[r];
    const uint32_t t = light_slot(run.n, rc);
    return run.start + light_select_slot(g.run_slots[run.start + t], t, rb);
}

/* ---- the host's builders (the device pass of hipcc parses them too and emits nothing) */
inline bool grid_finite(float v) { return v == v && v >= -kFltMax && v <= kFltMax; }
inline float grid_size_of(float lo, float hi, int N) { return hi > lo ? (hi - lo) / (float)N : 1.0f; }
inline float grid_inv_of(float lo, float hi, int N) { return hi > lo ? (float)N / (hi - lo) : 1.0f; }

struct GridBox
{
    float lo[3], hi[3];
    bool any = false;
    void add(const float* v) /* one vertex: each finite coordinate on its own */
    {
        for (int a = 0; a < 3; ++a)
        {
            if (!grid_finite(v[a])) continue;
            if (!any_axis[a]) { lo[a] = hi[a] = v[a]; any_axis[a] = true; }
            else { if (v[a] < lo[a]) lo[a] = v[a]; if (v[a] > hi[a]) hi[a] = v[a]; }
        }
    }
    void close() /* an axis without a finite coordinate: [0, 0] */
    {
        for (int a = 0; a < 3; ++a)
            if (!any_axis[a]) lo[a] = hi[a] = 0.0f;
    }
    bool any_axis[3] = {false, false, false};
};

inline uint32_t grid_morton_part(uint32_t v) /* 10 bits, two zeros between neighbours */
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

struct LightGrid
{
    int N = 0;
    uint32_t B = 0, L = 0; /* B = B' */
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, size[3] = {1, 1, 1}, inv[3] = {1, 1, 1};
    float h = 0.0f;
    std::vector<uint32_t> perm, cluster_of; /* perm[pos] = light; cluster_of[light] = run */
    std::vector<GridRun> runs;
    std::vector<AliasSlot> run_slots; /* position order */
    std::vector<uint64_t> run_K;      /* position order, out of n_r 2^23 */
    std::vector<double> P;
    std::vector<float> centre;        /* 3 per run */
    std::vector<float> rho;
    std::vector<float> cell_w;        /* N^3 x B' */
    std::vector<AliasSlot> cells;
    std::vector<uint64_t> cell_K;     /* out of B' 2^23 */
    bool ok = false;                  /* some run has P > 0 */

    GridBounds bounds() const { return GridBounds{F3(lo[0], lo[1], lo[2]), F3(inv[0], inv[1], inv[2]), N}; }
    size_t cell_slots() const { return (size_t)N * (size_t)N * (size_t)N * (size_t)B; }
};

/* bounds of `n` triangles of `stride` floats each (the first 9: v0, v1, v2) */
inline void grid_build_bounds(LightGrid& g, const float* tris, size_t stride, size_t n, int N)
{
    GridBox box;
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) box.add(tris + stride * i + 3 * k);
    box.close();
    g.N = N;
    for (int a = 0; a < 3; ++a)
    {
        g.lo[a] = box.lo[a]; g.hi[a] = box.hi[a];
        g.size[a] = grid_size_of(box.lo[a], box.hi[a], N);
        g.inv[a] = grid_inv_of(box.lo[a], box.hi[a], N);
    }
    g.h = 0.5f * length(F3(g.size[0], g.size[1], g.size[2]));
}

/* runs of the L lights `ids` (triangle indices into `tris`) with the weights `w` (light_weight, light list order) */
inline void grid_build_runs(LightGrid& g, const float* tris, size_t stride, const uint32_t* ids, const float* w, uint32_t L, int clusters)
{
    g.L = L;
    g.B = L < (uint32_t)clusters ? L : (uint32_t)clusters;
    const uint32_t B = g.B;
    g.perm.assign(L, 0u); g.cluster_of.assign(L, 0u);
    g.runs.assign(B, GridRun{0u, 0u});
    g.run_slots.assign(L, AliasSlot{0u, 0u}); g.run_K.assign(L, 0u);
    g.P.assign(B, 0.0); g.centre.assign((size_t)3 * B, 0.0f); g.rho.assign(B, 0.0f);
    g.ok = false;
    if (L == 0) return;
    GridBox lb;
    for (uint32_t i = 0; i < L; ++i)
        for (int k = 0; k < 3; ++k) lb.add(tris + stride * (size_t)ids[i] + 3 * k);
    lb.close();
    float linv[3];
    for (int a = 0; a < 3; ++a) linv[a] = grid_inv_of(lb.lo[a], lb.hi[a], 1024);
    std::vector<std::pair<uint32_t, uint32_t>> order(L);
    for (uint32_t i = 0; i < L; ++i)
    {
        const float* t = tris + stride * (size_t)ids[i];
        const f3 c = ((F3(t[0], t[1], t[2]) + F3(t[3], t[4], t[5])) + F3(t[6], t[7], t[8])) * (1.0f / 3.0f);
        const uint32_t qx = (uint32_t)grid_axis_cell(c.x, lb.lo[0], linv[0], 1024), qy = (uint32_t)grid_axis_cell(c.y, lb.lo[1], linv[1], 1024),
                       qz = (uint32_t)grid_axis_cell(c.z, lb.lo[2], linv[2], 1024);
        order[i] = std::make_pair(grid_morton_part(qx) | (grid_morton_part(qy) << 1) | (grid_morton_part(qz) << 2), i);
    }
    std::sort(order.begin(), order.end()); /* by code, then by light index */
    for (uint32_t p = 0; p < L; ++p) g.perm[p] = order[p].second;
    std::vector<float> rw;
    std::vector<AliasSlot> slots;
    std::vector<uint64_t> K;
    for (uint32_t r = 0; r < B; ++r)
    {
        const uint32_t a = (uint32_t)((uint64_t)r * L / B), b = (uint32_t)((uint64_t)(r + 1u) * L / B);
        g.runs[r] = GridRun{a, b - a};
        rw.resize(b - a);
        GridBox rb;
        double P = 0.0;
        for (uint32_t p = a; p < b; ++p)
        {
            const uint32_t i = g.perm[p];
            g.cluster_of[i] = r;
            rw[p - a] = w[i];
            if (light_weight_ok(w[i])) P += (double)w[i];
            for (int k = 0; k < 3; ++k) rb.add(tris + stride * (size_t)ids[i] + 3 * k);
        }
        rb.close();
        const f3 c = F3(0.5f * (rb.lo[0] + rb.hi[0]), 0.5f * (rb.lo[1] + rb.hi[1]), 0.5f * (rb.lo[2] + rb.hi[2]));
        float rho = 0.0f;
        for (uint32_t p = a; p < b; ++p)
            for (int k = 0; k < 3; ++k)
            {
                const float* v = tris + stride * (size_t)ids[g.perm[p]] + 3 * k;
                if (!grid_finite(v[0]) || !grid_finite(v[1]) || !grid_finite(v[2])) continue;
                const float d = length(F3(v[0], v[1], v[2]) - c);
                if (d > rho) rho = d;
            }
        g.P[r] = P; g.rho[r] = rho;
        g.centre[3 * (size_t)r] = c.x; g.centre[3 * (size_t)r + 1] = c.y; g.centre[3 * (size_t)r + 2] = c.z;
        if (alias_build(rw.data(), b - a, slots, K)) g.ok = true;
        for (uint32_t p = a; p < b; ++p) { g.run_slots[p] = slots[p - a]; g.run_K[p] = K[p - a]; }
    }
}

/* weight of run r in the cell with the centre xc (header comment) */
inline float grid_cell_weight(double P, const float* xc, const float* cr, float h, float rho)
{
    if (!(P > 0.0)) return 0.0f;
    const double dx = (double)xc[0] - (double)cr[0], dy = (double)xc[1] - (double)cr[1], dz = (double)xc[2] - (double)cr[2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    const double m = ((double)h + (double)rho) * ((double)h + (double)rho);
    const double q = P / (d2 > m ? d2 : m);
    if (!(q >= (double)kGridFltMin)) return kGridFltMin;
    if (q > (double)kFltMax) return kFltMax;
    return (float)q;
}

/* the cells' tables from the bounds and the runs */
inline void grid_build_cells(LightGrid& g)
{
    const size_t n = g.cell_slots();
    g.cell_w.assign(n, 0.0f); g.cells.assign(n, AliasSlot{0u, 0u}); g.cell_K.assign(n, 0u);
    if (g.B == 0) return;
    const int N = g.N;
    const uint32_t B = g.B;
    std::vector<AliasSlot> slots;
    std::vector<uint64_t> K;
    for (int cz = 0; cz < N; ++cz)
        for (int cy = 0; cy < N; ++cy)
            for (int cx = 0; cx < N; ++cx)
            {
                const size_t base = ((size_t)(cz * N + cy) * N + cx) * B;
                const float xc[3] = {g.lo[0] + ((float)cx + 0.5f) * g.size[0], g.lo[1] + ((float)cy + 0.5f) * g.size[1], g.lo[2] + ((float)cz + 0.5f) * g.size[2]};
                for (uint32_t r = 0; r < B; ++r) g.cell_w[base + r] = grid_cell_weight(g.P[r], xc, &g.centre[3 * (size_t)r], g.h, g.rho[r]);
                alias_build(&g.cell_w[base], B, slots, K);
                for (uint32_t r = 0; r < B; ++r) { g.cells[base + r] = slots[r]; g.cell_K[base + r] = K[r]; }
            }
}

inline void grid_build(LightGrid& g, const float* tris, size_t stride, size_t n_tris, const uint32_t* ids, const float* w, uint32_t L, int N, int clusters)
{
    grid_build_bounds(g, tris, stride, n_tris, N);
    grid_build_runs(g, tris, stride, ids, w, L, clusters);
    grid_build_cells(g);
}

}  // namespace rt
