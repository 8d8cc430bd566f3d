"""CPU restatement of rt_light_grid (csrc/light_grid.h), for tests/test_light_grid_cpu.py and
tests/test_gpu_light_grid.py: the bounds, the runs, the cells' tables with their realised counts, the selection, and generate_candidate
(10_restir_di.cu:36-135) with its light drawn from the grid.

Plain C++ appended to the program of tests/light_sampling_ref.py (the reference's PODs, the surface point, the brute-force shadow ray
and the light list are that file's), compiled with `g++ -ffp-contract=off` from csrc/light_grid.h, csrc/light_alias.h and
csrc/rt_device.h, the headers the kernel and the library's host code are compiled from: the records equal the GPU's bit for bit. A
candidate draws rv0, ra, rc, rb, bx, by, u. With the grid off the function is light_sampling_ref's, which the CPU tests anchor to the
oracle. make_lamp_field() is the scene the mode was specified on."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import light_sampling_ref as ls

ROOT, CSRC = ls.ROOT, ls.CSRC
ONE = ls.ONE
UNIFORM, POWER, GRID = 0, 1, 2

PROGRAM = ls.PROGRAM + r"""
#include "light_grid.h"

struct Grid
{
    LightGrid g;
    std::vector<uint32_t> ids;
    std::vector<float> w;
    std::vector<float> cell_prob, run_prob; /* what the device's tables hold: binary32 */
    GridView view() const { return GridView{g.bounds(), g.B, g.cells.data(), cell_prob.data(), g.runs.data(), g.run_slots.data()}; }
};
extern "C" void* lg_new(const Tri* tris, int n_tris, int N, int clusters)
{
    Grid* G = new Grid;
    G->ids.resize((size_t)n_tris + 1); G->w.resize((size_t)n_tris + 1);
    const uint32_t L = (uint32_t)ls_lights(tris, n_tris, G->ids.data(), G->w.data());
    G->ids.resize(L); G->w.resize(L);
    grid_build(G->g, (const float*)tris, 15, (size_t)n_tris, G->ids.data(), G->w.data(), L, N, clusters);
    const LightGrid& g = G->g;
    G->cell_prob.resize(L ? g.cell_slots() : 0); G->run_prob.resize(L);
    for (size_t k = 0; k < G->cell_prob.size(); ++k) G->cell_prob[k] = light_select_prob(g.cell_K[k], g.B);
    for (uint32_t r = 0; r < g.B; ++r)
        for (uint32_t p = g.runs[r].start; p < g.runs[r].start + g.runs[r].n; ++p) G->run_prob[p] = light_select_prob(g.run_K[p], g.runs[r].n);
    return G;
}
extern "C" void lg_free(void* h) { delete (Grid*)h; }
/* out: N, B', L, ok */
extern "C" void lg_sizes(void* h, uint32_t* out)
{
    const LightGrid& g = ((Grid*)h)->g;
    out[0] = (uint32_t)g.N; out[1] = g.B; out[2] = g.L; out[3] = g.ok ? 1u : 0u;
}
/* bounds: lo, hi, size, inv, then h (13 floats); the per-light, per-run and per-cell-slot arrays */
extern "C" void lg_get(void* h, float* bounds, uint32_t* ids, float* w, uint32_t* perm, uint32_t* cluster_of, uint32_t* run_start, uint32_t* run_thr,
                       uint32_t* run_alias, uint64_t* run_K, double* P, float* centre, float* rho, float* cell_w, uint32_t* cell_thr,
                       uint32_t* cell_alias, uint64_t* cell_K, float* cell_prob, float* run_prob)
{
    const Grid* G = (Grid*)h;
    const LightGrid& g = G->g;
    for (int a = 0; a < 3; ++a) { bounds[a] = g.lo[a]; bounds[3 + a] = g.hi[a]; bounds[6 + a] = g.size[a]; bounds[9 + a] = g.inv[a]; }
    bounds[12] = g.h;
    for (uint32_t i = 0; i < g.L; ++i)
    {
        ids[i] = G->ids[i]; w[i] = G->w[i]; perm[i] = g.perm[i]; cluster_of[i] = g.cluster_of[i];
        run_thr[i] = g.run_slots[i].thr; run_alias[i] = g.run_slots[i].alias; run_K[i] = g.run_K[i]; run_prob[i] = G->run_prob[i];
    }
    for (uint32_t r = 0; r < g.B; ++r)
    {
        run_start[r] = g.runs[r].start; P[r] = g.P[r]; rho[r] = g.rho[r];
        for (int a = 0; a < 3; ++a) centre[3 * r + a] = g.centre[3 * (size_t)r + a];
    }
    run_start[g.B] = g.L;
    for (size_t k = 0; k < G->cell_prob.size(); ++k)
    {
        cell_w[k] = g.cell_w[k]; cell_thr[k] = g.cells[k].thr; cell_alias[k] = g.cells[k].alias; cell_K[k] = g.cell_K[k]; cell_prob[k] = G->cell_prob[k];
    }
}
extern "C" void lg_cell_of(void* h, const float* p, int n, uint32_t* out)
{
    const GridBounds b = ((Grid*)h)->g.bounds();
    for (int i = 0; i < n; ++i) out[i] = grid_cell_of(b, F3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
}
/* one selection: the light (light list order); out: run, sorted position; prob: the cell's factor */
extern "C" uint32_t lg_select(void* h, uint32_t cell, float rv0, float ra, float rc, float rb, uint32_t* out, float* prob)
{
    const Grid* G = (Grid*)h;
    const uint32_t pos = grid_select(G->view(), cell, rv0, ra, rc, rb, *prob);
    out[0] = G->g.cluster_of[G->g.perm[pos]]; out[1] = pos;
    return G->g.perm[pos];
}
/* light_select_slot over all 2^23 values PCG::uniformf can give: the cell's slot s (counts per run), the run's slot t (counts per
 * sorted position of the run) */
extern "C" void lg_cell_slot_all(void* h, uint32_t cell, uint32_t s, uint64_t* counts)
{
    const LightGrid& g = ((Grid*)h)->g;
    for (uint32_t k = 0; k < (1u << 23); ++k)
        counts[light_select_slot(g.cells[(size_t)cell * g.B + s], s, pm_u2f(k | 0x3f800000u) - 1.0f)] += 1u;
}
extern "C" void lg_run_slot_all(void* h, uint32_t r, uint32_t t, uint64_t* counts)
{
    const LightGrid& g = ((Grid*)h)->g;
    for (uint32_t k = 0; k < (1u << 23); ++k)
        counts[light_select_slot(g.run_slots[g.runs[r].start + t], t, pm_u2f(k | 0x3f800000u) - 1.0f)] += 1u;
}

extern "C" int lg_generate(void* h, int W, int H, int frame, const Tri* tris, int n_tris, const Vis* vis, const float* eye3, int ris_sample_count,
                           int shadowed, int vis_reuse, Reservoir* out)
{
    const Grid* G = (Grid*)h;
    const LightGrid& g = G->g;
    const GridView V = G->view();
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
    if ((g.L == 0 || !g.ok) && ris_sample_count > 0) return 1;
#pragma omp parallel for schedule(dynamic, 2)
    for (int row = 0; row < H; ++row)
        for (int xi = 0; xi < W; ++xi)
        {
            const int yi = H - 1 - row;
            const size_t q = (size_t)xi + (size_t)row * W;
            Reservoir r;
            memset(&r, 0, sizeof(r));
            if (vis[q].index == -1 || emissive(tris[vis[q].index])) { out[q] = r; continue; }
            f3 sp, sn;
            surface(tris, vis[q], eye, sp, sn);
            const uint32_t cell = grid_cell_of(V.b, sp);
            PCG rng = pcg_init(hashPCG4((uint32_t)xi, (uint32_t)yi, (uint32_t)frame, 0u), 0);
            for (int i = 0; i < ris_sample_count; ++i)
            {
                const float rv0 = rng.uniformf();
                const float ra = rng.uniformf();
                const float rc = rng.uniformf();
                const float rb = rng.uniformf();
                float cell_prob;
                const uint32_t pos = grid_select(V, cell, rv0, ra, rc, rb, cell_prob);
                float bx = rng.uniformf();
                float by = rng.uniformf();
                const Tri& lt = tris[G->ids[g.perm[pos]]];
                const f3 v0 = v3(lt.v), v1 = v3(lt.v + 3), v2 = v3(lt.v + 6);
                warp_unit_triangle(bx, by);
                const f3 lp = (1.0f - bx - by) * v0 + bx * v1 + by * v2;
                const f3 ln = tri_normal(v0, v1, v2);
                const float pdf = grid_pdf(cell_prob, G->run_prob[pos] * 1.0f / tri_area(v0, v1, v2));
                const float p_hat = target_unshadowed(sp, sn, lp, ln, luminance(v3(lt.emissive))); /* unshadowed always (:104) */
                const float weight = p_hat / pdf;
                const float u = rng.uniformf();
                r.w_sum += weight;
                r.M += 1;
                if (u < weight / r.w_sum)
                {
                    put(r.origin_position, sp); put(r.origin_normal, sn); put(r.hit_position, lp); put(r.hit_normal, ln);
                    memcpy(r.radiance, lt.emissive, 12);
                    r.visibility = 0;
                }
            }
            const f3 hp = v3(r.hit_position), hn = v3(r.hit_normal);
            const float lum = luminance(v3(r.radiance));
            float p_hat;
            if (shadowed) p_hat = (1.0f / kPI) * geometry_term(sp, sn, hp, hn) * (check_visibility(tris, n_tris, sp, sn, hp) ? 1.0f : 0.0f) * lum;
            else p_hat = target_unshadowed(sp, sn, hp, hn, lum);
            r.ucw = p_hat > 0.0f ? r.w_sum / ((float)r.M * p_hat) : 0.0f;
            if (vis_reuse) r.visibility = check_visibility(tris, n_tris, sp, sn, hp) ? 1 : 0;
            out[q] = r;
        }
    return 0;
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="light_grid_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci, u32, f = C.c_void_p, C.c_int, C.c_uint32, C.c_float
        L.lg_new.argtypes = [vp, ci, ci, ci]
        L.lg_new.restype = vp
        L.lg_free.argtypes = [vp]
        L.lg_sizes.argtypes = [vp, vp]
        L.lg_get.argtypes = [vp] * 19
        L.lg_cell_of.argtypes = [vp, vp, ci, vp]
        L.lg_select.argtypes = [vp, u32, f, f, f, f, vp, vp]
        L.lg_select.restype = u32
        L.lg_cell_slot_all.argtypes = [vp, u32, u32, vp]
        L.lg_run_slot_all.argtypes = [vp, u32, u32, vp]
        L.lg_generate.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, ci, ci, ci, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Grid:
    """the tables of rt_light_grid(cells, clusters) for the triangles `tris`, as csrc/light_grid.h builds them. Attributes: N, B (the
    clusters built), L, ok; lo / hi / size / inv / h; ids, w (light list order); perm, cluster_of; run_start (B + 1), run_thr /
    run_alias / run_K / run_prob (sorted position); P, centre, rho (per run); cell_w / cell_thr / cell_alias / cell_K / cell_prob
    (N^3 x B, cell-major)."""

    def __init__(self, tris, cells, clusters):
        tris = np.ascontiguousarray(tris)
        assert tris.dtype.itemsize == 60
        self.tris = tris
        self.h = lib().lg_new(_p(tris), len(tris), int(cells), int(clusters))
        s = np.zeros(4, np.uint32)
        lib().lg_sizes(self.h, _p(s))
        self.N, self.B, self.L, self.ok = int(s[0]), int(s[1]), int(s[2]), bool(s[3])
        L, B = self.L, self.B
        n = self.N ** 3 * B if L else 0
        u32, u64, f32 = np.uint32, np.uint64, np.float32
        b = np.zeros(13, f32)
        self.ids, self.w, self.perm, self.cluster_of = np.zeros(L, u32), np.zeros(L, f32), np.zeros(L, u32), np.zeros(L, u32)
        self.run_start, self.run_thr, self.run_alias, self.run_K = np.zeros(B + 1, u32), np.zeros(L, u32), np.zeros(L, u32), np.zeros(L, u64)
        self.P, self.centre, self.rho = np.zeros(B, np.float64), np.zeros((B, 3), f32), np.zeros(B, f32)
        self.cell_w, self.cell_thr, self.cell_alias = np.zeros(n, f32), np.zeros(n, u32), np.zeros(n, u32)
        self.cell_K, self.cell_prob, self.run_prob = np.zeros(n, u64), np.zeros(n, f32), np.zeros(L, f32)
        lib().lg_get(self.h, _p(b), _p(self.ids), _p(self.w), _p(self.perm), _p(self.cluster_of), _p(self.run_start), _p(self.run_thr),
                     _p(self.run_alias), _p(self.run_K), _p(self.P), _p(self.centre), _p(self.rho), _p(self.cell_w), _p(self.cell_thr),
                     _p(self.cell_alias), _p(self.cell_K), _p(self.cell_prob), _p(self.run_prob))
        self.lo, self.hi, self.size, self.inv, self.hdiag = b[0:3].copy(), b[3:6].copy(), b[6:9].copy(), b[9:12].copy(), b[12]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.lg_free(self.h)
            self.h = None

    def cell_of(self, points):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.zeros(len(p), np.uint32)
        lib().lg_cell_of(self.h, _p(p), len(p), _p(out))
        return out

    def select(self, cell, rv0, ra, rc, rb):
        """(light, run, sorted position, the cell's binary32 factor of the pdf)"""
        out, prob = np.zeros(2, np.uint32), np.zeros(1, np.float32)
        f = C.c_float
        i = lib().lg_select(self.h, int(cell), f(rv0), f(ra), f(rc), f(rb), _p(out), _p(prob))
        return int(i), int(out[0]), int(out[1]), prob[0]

    def cell_slot_all(self, cell, s):
        counts = np.zeros(self.B, np.uint64)
        lib().lg_cell_slot_all(self.h, int(cell), int(s), _p(counts))
        return counts

    def run_slot_all(self, r, t):
        counts = np.zeros(int(self.run_start[r + 1] - self.run_start[r]), np.uint64)
        lib().lg_run_slot_all(self.h, int(r), int(t), _p(counts))
        return counts


def generate_candidate(W, H, frame, tris, vis, eye, opt, mode, res=None, grid=None):
    """generate_candidate over the whole image; mode UNIFORM / POWER: tests/light_sampling_ref.py's; GRID: with the light drawn from
    `grid` (a Grid of the same triangles). Raises where the library returns RT_ERR_STATE."""
    if mode != GRID:
        return ls.generate_candidate(W, H, frame, tris, vis, eye, opt, mode, res)
    tris, vis = np.ascontiguousarray(tris), np.ascontiguousarray(vis)
    assert tris.dtype.itemsize == 60 and vis.dtype.itemsize == 16 and len(vis) == W * H and grid is not None and len(grid.tris) == len(tris)
    if res is None:
        from oracle import binding as ob

        res = np.zeros(W * H, dtype=ob.RESERVOIR)
    assert res.dtype.itemsize == 76 and len(res) == W * H and res.flags.c_contiguous
    e = np.ascontiguousarray(eye, dtype=np.float32)
    rc = lib().lg_generate(grid.h, W, H, int(frame), _p(tris), len(tris), _p(vis), _p(e), int(opt["ris_sample_count"][0]),
                           int(opt["use_shadowed_target_function"][0]), int(opt["use_visibility_reuse"][0]), _p(res))
    if rc:
        raise RuntimeError("no light can be selected")
    return res


FIELD_EYE, FIELD_AT = (0.0, 6.0, 14.0), (0.0, 0.0, 0.0)


def make_lamp_field(triangle_dtype=None):
    """a 20 x 20 floor, 16 x 16 square lamps of side 0.3 at height 2 facing down (Ke = 10: 512 emissive triangles of equal power) and
    four boxes on the floor, so that visibility matters. 562 triangles; view: FIELD_EYE -> FIELD_AT."""
    from cedec_2024_rt_amd.types import TRIANGLE

    quads = [([(-10.0, 0.0, -10.0), (-10.0, 0.0, 10.0), (10.0, 0.0, 10.0), (10.0, 0.0, -10.0)], 0.0)]
    for j in range(16):
        for i in range(16):
            x, z = -9.375 + 1.25 * i - 0.15, -9.375 + 1.25 * j - 0.15
            quads.append(([(x, 2.0, z), (x + 0.3, 2.0, z), (x + 0.3, 2.0, z + 0.3), (x, 2.0, z + 0.3)], 10.0))
    for cx, cz, s, hgt in ((-4.0, -3.0, 1.0, 1.2), (3.5, -5.0, 0.8, 1.6), (5.0, 3.0, 1.2, 0.9), (-2.5, 4.5, 0.7, 1.5)):
        x0, x1, z0, z1 = cx - s, cx + s, cz - s, cz + s
        quads.append(([(x0, hgt, z0), (x0, hgt, z1), (x1, hgt, z1), (x1, hgt, z0)], 0.0))  # top
        quads.append(([(x0, 0.0, z1), (x1, 0.0, z1), (x1, hgt, z1), (x0, hgt, z1)], 0.0))
        quads.append(([(x1, 0.0, z0), (x0, 0.0, z0), (x0, hgt, z0), (x1, hgt, z0)], 0.0))
        quads.append(([(x0, 0.0, z0), (x0, 0.0, z1), (x0, hgt, z1), (x0, hgt, z0)], 0.0))
        quads.append(([(x1, 0.0, z1), (x1, 0.0, z0), (x1, hgt, z0), (x1, hgt, z1)], 0.0))
    t = np.zeros(2 * len(quads), dtype=triangle_dtype or TRIANGLE)
    for k, (q, ke) in enumerate(quads):
        q = np.array(q, np.float32)
        t["v"][2 * k], t["v"][2 * k + 1] = q[[0, 1, 2]], q[[0, 2, 3]]
        t["color"][2 * k:2 * k + 2], t["emissive"][2 * k:2 * k + 2] = 0.8, np.float32(ke)
    return t
