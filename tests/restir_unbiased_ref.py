"""CPU restatement of the unbiased spatial pass (rt_spatial_unbiased; csrc/frame_kernels.h, k_spatial_unbiased)
for tests/test_restir_unbiased_cpu.py and tests/test_gpu_restir_unbiased.py.

One pass over the whole image in plain C++ on the reference's 76-byte Reservoir records (buffer index = row * W + x). Every formula
comes from csrc/rt_device.h and csrc/portable_math.h, the headers the kernel is compiled from; built with `g++ -ffp-contract=off`,
so the result equals the GPU's bit for bit (rows run on OpenMP threads: a pixel is computed by one thread). Visibility is brute-force
any-hit over all triangles with intersect_ray_triangle: the BVH walk equals brute force (csrc/bvh_cull.h has the argument,
tests/test_gpu_targeted_rays.py the rays that would show otherwise).
mode = REFERENCE makes it the reference's pass (10_restir_di.cu:256-388, unshadowed target function), which anchors the restatement
to oracle.Scene.spatial_resampling. diag holds per pixel {Z, M_sum, mask of neighbours k with Mk > 0 that geometry alone kept out
of Z, mask of those the shadow ray alone kept out}; in reference mode Z = M_sum and the masks are 0."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

REFERENCE, UNBIASED = 0, 1

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "rt_device.h"
using namespace rt;

struct Tri { float v[9], color[3], emissive[3]; };
struct Vis { float u, v; int32_t index, pad; };
struct Reservoir
{
    float origin_position[3], origin_normal[3], hit_position[3], hit_normal[3], radiance[3];
    uint8_t visibility, pad[3];
    float w_sum, ucw;
    int32_t M;
};
static_assert(sizeof(Tri) == 60 && sizeof(Vis) == 16 && sizeof(Reservoir) == 76, "the reference's PODs");

static f3 v3(const float* a) { return F3(a[0], a[1], a[2]); }
static bool emissive(const Tri& t) { return t.emissive[0] > 0.0f || t.emissive[1] > 0.0f || t.emissive[2] > 0.0f; }
static bool shaded(const Tri* tris, const Vis& v) { return v.index != -1 && !emissive(tris[v.index]); }
/* common/core.hpp:189-207 */
static void surface(const Tri* tris, const Vis& v, f3 eye, f3& p, f3& n)
{
    const Tri& t = tris[v.index];
    const f3 v0 = v3(t.v), v1 = v3(t.v + 3), v2 = v3(t.v + 6);
    p = (1.0f - v.u - v.v) * v0 + v.u * v1 + v.v * v2;
    n = tri_normal(v0, v1, v2);
    if (dot(normalize(eye - p), n) < 0.0f) n = -n;
}
/* common/raytrace.hpp:45-52: any hit decides, so the order of the triangles does not matter */
static bool check_visibility(const Tri* tris, int n_tris, f3 p0, f3 n0, f3 p1)
{
    const f3 org = p0 + 0.001f * n0, dir = p1 - p0;
    for (int i = 0; i < n_tris; ++i)
    {
        float t, u, v;
        if (intersect_ray_triangle(t, u, v, org, dir, 0.0f, 0.99f, v3(tris[i].v), v3(tris[i].v + 3), v3(tris[i].v + 6))) return false;
    }
    return true;
}
static void take_sample(Reservoir& r, const Reservoir& o)
{
    memcpy(r.origin_position, o.origin_position, 15 * sizeof(float));
    r.visibility = o.visibility;
    memcpy(r.pad, o.pad, 3);
}

extern "C" void ru_spatial(int W, int H, int frame, int pass, const Tri* tris, int n_tris, const Vis* vis, const float* eye3, int use_spatial,
                           int count, float radius, int vis_reuse, int mode, const Reservoir* in, Reservoir* out, int32_t* diag)
{
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
#pragma omp parallel for schedule(dynamic, 2)
    for (int row = 0; row < H; ++row)
        for (int xi = 0; xi < W; ++xi)
        {
            const int yi = H - 1 - row;
            const size_t q = (size_t)xi + (size_t)row * W;
            int32_t* D = diag + 4 * q;
            D[0] = D[1] = D[2] = D[3] = 0;
            if (!shaded(tris, vis[q])) continue; /* the reference stores nothing here (:275-287) */
            f3 sp, sn;
            surface(tris, vis[q], eye, sp, sn);
            PCG rng = pcg_init(hashPCG4((uint32_t)xi, (uint32_t)yi, (uint32_t)frame, (uint32_t)(2 + pass)), 0);
            Reservoir r = in[q];
            if (!use_spatial) { out[q] = r; continue; }
            if (mode == 1)
                r.w_sum = unbiased_weight(sp, sn, v3(r.hit_position), v3(r.hit_normal), luminance(v3(r.radiance)), 1.0f, r.ucw, r.M);
            int Z = r.M;
            f3 np[5], nn[5];
            int Mk[5] = {0, 0, 0, 0, 0};
            const float scale = radius / 1.96f;
            for (int k = 0; k < count; ++k)
            {
                const float rv0 = rng.uniformf();
                const float rv1 = rng.uniformf();
                /* common/reservoir.hpp:89-95 */
                const float rad = sqrt_guarded(fmax_dev(-2.0f * pm_logf(rv0), 0.0f));
                const float phi = 2.0f * kPI * rv1;
                float sn_phi, cs_phi;
                pm_sincosf(phi, &sn_phi, &cs_phi);
                const int x = f2i_sat((float)xi + scale * (rad * cs_phi));
                const int y = f2i_sat((float)yi + scale * (rad * sn_phi));
                if (x < 0 || x >= W || y < 0 || y >= H) continue;
                if (x == xi && y == yi) continue;
                const size_t pid = (size_t)x + (size_t)(H - y - 1) * W;
                if (!shaded(tris, vis[pid])) continue;
                Reservoir n = in[pid];
                const f3 hp = v3(n.hit_position), hn = v3(n.hit_normal);
                const float lum = luminance(v3(n.radiance));
                float weight;
                int M;
                if (mode == 1)
                {
                    f3 p, nrm;
                    surface(tris, vis[pid], eye, p, nrm);
                    M = scale_M(n.M, rejection_heuristics(sp, sn, p, nrm, eye));
                    weight = unbiased_weight(sp, sn, hp, hn, lum, (vis_reuse && !n.visibility) ? 0.0f : 1.0f, n.ucw, M);
                    if (k < 5) { np[k] = p; nn[k] = nrm; Mk[k] = M; }
                }
                else
                {
                    float p_hat_y = target_unshadowed(sp, sn, hp, hn, lum);
                    if (vis_reuse) p_hat_y *= (float)n.visibility;
                    M = scale_M(n.M, rejection_heuristics(v3(r.origin_position), v3(r.origin_normal), v3(n.origin_position), v3(n.origin_normal), eye));
                    weight = p_hat_y * n.ucw * (float)M;
                }
                const float u = rng.uniformf();
                r.w_sum += weight;
                r.M += M;
                if (reservoir_accept(u, weight, r.w_sum)) take_sample(r, n);
            }
            const f3 y = v3(r.hit_position), yn = v3(r.hit_normal);
            const float p_hat = target_unshadowed(sp, sn, y, yn, luminance(v3(r.radiance)));
            if (mode == 1)
            {
                for (int k = 0; k < 5; ++k)
                {
                    if (Mk[k] <= 0) continue;
                    if (!unbiased_in_support(np[k], nn[k], y, yn)) { D[2] |= 1 << k; continue; }
                    if (vis_reuse && !check_visibility(tris, n_tris, np[k], nn[k], y)) { D[3] |= 1 << k; continue; }
                    Z += Mk[k];
                }
                r.ucw = unbiased_ucw(r.w_sum, Z, p_hat);
                if (vis_reuse) r.visibility = check_visibility(tris, n_tris, sp, sn, y) ? 1 : 0;
            }
            else
            {
                Z = r.M;
                r.ucw = p_hat > 0.0f ? r.w_sum / ((float)r.M * p_hat) : 0.0f;
            }
            D[0] = Z; D[1] = r.M;
            out[q] = r;
        }
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="restir_unbiased_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.ru_spatial.argtypes = [ci, ci, ci, ci, vp, ci, vp, vp, ci, ci, C.c_float, ci, ci, vp, vp, vp]
        L.ru_spatial.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


LEDGE_EYE, LEDGE_AT = (-1.0, 4.0, 7.0), (1.5, 0.3, 0.0)


def make_ledge(triangle_dtype):
    """A scene where the geometry term alone keeps neighbours out of Z. The reference's term takes |cos| at both ends, so it is zero
    only for a sample exactly in the neighbour's plane: here a lamp lies IN the floor (y = 0, the floor's quads leave its square
    free) next to a ramp that rises by 1.5 over 4 (20.6 degrees: the rejection heuristics keep 0.59 of a floor neighbour's M). Ramp
    pixels select the floor lamp; for their floor neighbours sample and surface both have y = 0 exactly, the direction's y is 0, the
    normal is (0, 1, 0), and G = 0 in binary32. A second lamp overhead lights the floor. 22 triangles; view: LEDGE_EYE -> LEDGE_AT."""
    quads = []
    xs, zs = (-6.0, -1.0, 1.0, 2.0), (-6.0, -1.0, 1.0, 6.0)
    for i in range(3):
        for j in range(3):
            q = [(xs[i], 0, zs[j]), (xs[i + 1], 0, zs[j]), (xs[i + 1], 0, zs[j + 1]), (xs[i], 0, zs[j + 1])]
            quads.append((q, 0.0, 12.0) if i == j == 1 else (q, 0.7, 0.0))
    quads.append(([(2, 0, -6), (6, 1.5, -6), (6, 1.5, 6), (2, 0, 6)], 0.7, 0.0))
    quads.append(([(-3.5, 5, -0.5), (-2.5, 5, -0.5), (-2.5, 5, 0.5), (-3.5, 5, 0.5)], 0.0, 20.0))
    t = np.zeros(2 * len(quads), dtype=triangle_dtype)
    for i, (q, col, ke) in enumerate(quads):
        q = np.array(q, np.float32)
        t["v"][2 * i], t["v"][2 * i + 1] = q[[0, 1, 2]], q[[0, 2, 3]]
        t["color"][2 * i:2 * i + 2], t["emissive"][2 * i:2 * i + 2] = col, ke
    return t


def spatial(W, H, frame, pas, tris, vis, eye, opt, rin, mode=UNBIASED, rout=None):
    """One pass. tris / vis / opt / rin: the oracle's TRIANGLE / VISIBILITY / OPTIONS / RESERVOIR arrays. Pixels that are not shaded
    keep what rout held (zeros if rout is None), as in the reference. Returns (rout, diag) with diag (W * H, 4) int32."""
    assert not int(opt["use_shadowed_target_function"][0]), "unshadowed target function only"
    assert mode == REFERENCE or int(opt["spatial_resampling_sample_count"][0]) <= 5
    tris, vis, rin = np.ascontiguousarray(tris), np.ascontiguousarray(vis), np.ascontiguousarray(rin)
    assert tris.dtype.itemsize == 60 and vis.dtype.itemsize == 16 and rin.dtype.itemsize == 76 and len(rin) == W * H == len(vis)
    rout = np.zeros(W * H, dtype=rin.dtype) if rout is None else rout
    diag = np.zeros((W * H, 4), dtype=np.int32)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    lib().ru_spatial(W, H, int(frame), int(pas), _p(tris), len(tris), _p(vis), _p(e), int(opt["use_spatial_resampling"][0]),
                     int(opt["spatial_resampling_sample_count"][0]), C.c_float(np.float32(opt["spatial_resampling_radius"][0])),
                     int(opt["use_visibility_reuse"][0]), int(mode), _p(rin), _p(rout), _p(diag))
    return rout, diag
