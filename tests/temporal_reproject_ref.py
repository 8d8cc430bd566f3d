"""CPU restatement of the temporal merge with a reprojected history (rt_temporal_reprojection; csrc/temporal_reproject.h,
csrc/frame_kernels.h: load_prev_reprojected + temporal_merge) for tests/test_temporal_reproject_cpu.py and
tests/test_gpu_temporal_reproject.py.

One temporal_resampling over the whole image in plain C++ on the reference's 76-byte Reservoir records (buffer index = row * W + x).
Every formula comes from csrc/rt_device.h, csrc/portable_math.h and csrc/temporal_reproject.h, the headers the kernels are compiled
from; built with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit. Shadow rays are brute force over all triangles
with intersect_ray_triangle (the BVH walk equals brute force: csrc/bvh_cull.h).
mode = REFERENCE is the reference's merge (10_restir_di.cu:137-237: the history of pixel p is pixel p), which anchors the restatement
to oracle.Scene.temporal_resampling. mode = REPROJECT with the 36 bytes of the two RayGenerators equal is the same thing (the host
launches the same kernels); with other bytes a shaded pixel takes the record of the previous frame's pixel nearest to where its
surface point projects in the previous RayGenerator, Reservoir{} where there is none. diag holds per pixel {valid, xq, rq,
projected}: projected = the projection alone found a pixel inside the previous image, valid = and that pixel was shaded in the
previous Visibility buffer (its history is merged); (xq, rq) = the pixel, storage coordinates, 0 where not projected. In reference
mode and for pixels that are not shaded diag is {0, 0, 0, 0}."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

REFERENCE, REPROJECT = 0, 1

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "rt_device.h"
#include "temporal_reproject.h"
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
static float check_visibility(const Tri* tris, int n_tris, f3 p0, f3 n0, f3 p1)
{
    const f3 org = p0 + 0.001f * n0, dir = p1 - p0;
    for (int i = 0; i < n_tris; ++i)
    {
        float t, u, v;
        if (intersect_ray_triangle(t, u, v, org, dir, 0.0f, 0.99f, v3(tris[i].v), v3(tris[i].v + 3), v3(tris[i].v + 6))) return 0.0f;
    }
    return 1.0f;
}
/* common/reservoir.hpp:42-59 */
static float target(const Tri* tris, int n_tris, f3 sp, f3 sn, const Reservoir& r, int shadowed)
{
    const f3 hp = v3(r.hit_position), hn = v3(r.hit_normal);
    const float lum = luminance(v3(r.radiance));
    if (!shadowed) return target_unshadowed(sp, sn, hp, hn, lum);
    return (1.0f / kPI) * geometry_term(sp, sn, hp, hn) * check_visibility(tris, n_tris, sp, sn, hp) * lum;
}

/* rg_prev / rg_cur: 9 floats each {origin, right, up}; diag: 4 ints per pixel, see the module's text */
extern "C" void tr_temporal(int W, int H, int frame, const Tri* tris, int n_tris, const Vis* vis_cur, const Vis* vis_prev, const float* eye3,
                            const float* rg_prev, const float* rg_cur, int ris_sample_count, int use_temporal, int shadowed, int vis_reuse, int mode,
                            const Reservoir* hist, Reservoir* res, int32_t* diag)
{
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
    const bool gather = mode == 1 && !tr_same_camera(rg_prev, rg_cur);
    const size_t n_px = (size_t)W * (size_t)H;
#pragma omp parallel for schedule(dynamic, 2)
    for (int row = 0; row < H; ++row)
        for (int xi = 0; xi < W; ++xi)
        {
            const int yi = H - 1 - row;
            const size_t q = (size_t)xi + (size_t)row * W;
            int32_t* D = diag + 4 * q;
            D[0] = D[1] = D[2] = D[3] = 0;
            if (!shaded(tris, vis_cur[q])) continue;
            if (!use_temporal) continue;
            f3 sp, sn;
            surface(tris, vis_cur[q], eye, sp, sn);
            PCG rng = pcg_init(hashPCG4((uint32_t)xi, (uint32_t)yi, (uint32_t)frame, 1u), 0);
            Reservoir pr;
            if (!gather) pr = hist[q];
            else
            {
                memset(&pr, 0, sizeof(pr));
                const TrPixel t = tr_previous_pixel(sp, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H);
                if (t.valid)
                {
                    /* the index exists only behind the range test; the restatement aborts rather than read outside its buffers */
                    const size_t qi = (size_t)t.xq + (size_t)t.rq * W;
                    if (t.xq < 0 || t.xq >= W || t.rq < 0 || t.rq >= H || qi >= n_px) __builtin_trap();
                    D[1] = t.xq; D[2] = t.rq; D[3] = 1;
                    if (shaded(tris, vis_prev[qi])) { pr = hist[qi]; D[0] = 1; }
                }
            }
            Reservoir r = res[q];
            const int cap = 20 * ris_sample_count;
            pr.M = pr.M < cap ? pr.M : cap;
            float p_hat_y = target(tris, n_tris, sp, sn, pr, shadowed);
            if (vis_reuse) p_hat_y *= pr.visibility ? 1.0f : 0.0f;
            pr.M = scale_M(pr.M, rejection_heuristics(v3(r.origin_position), v3(r.origin_normal), v3(pr.origin_position), v3(pr.origin_normal), eye));
            const float weight = p_hat_y * pr.ucw * (float)pr.M;
            const float u = rng.uniformf();
            r.w_sum += weight;
            r.M += pr.M;
            if (reservoir_accept(u, weight, r.w_sum))
            {
                memcpy(r.origin_position, pr.origin_position, 15 * sizeof(float));
                r.visibility = pr.visibility;
                memcpy(r.pad, pr.pad, 3);
            }
            const float p_hat = target(tris, n_tris, sp, sn, r, shadowed);
            r.ucw = p_hat > 0.0f ? r.w_sum / ((float)r.M * p_hat) : 0.0f;
            res[q] = r;
        }
}

/* the projection alone, for the test against the float64 statement: per point {valid, xq, rq} and the continuous (px, pr) */
extern "C" void tr_project(int n, const float* points, const float* rg_prev, int W, int H, int32_t* pix, float* cont)
{
    for (int i = 0; i < n; ++i)
    {
        const f3 sp = v3(points + 3 * i);
        const TrPixel t = tr_previous_pixel(sp, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H);
        pix[3 * i] = t.valid; pix[3 * i + 1] = t.xq; pix[3 * i + 2] = t.rq;
        float px = NAN, pr = NAN;
        float a = 0.0f, b = 0.0f;
        const bool in = dn_reproject(sp, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H, a, b);
        /* dn_reproject sets the coordinates whenever the point is in front of the camera; recomputed here by its own expressions */
        const f3 R = v3(rg_prev + 3), U = v3(rg_prev + 6), d = sp - v3(rg_prev);
        const float tt = dot(d, normalize(cross(U, R)));
        if (tt > 0.0f)
        {
            const float ca = dot(d, R) / (tt * dot(R, R)), cb = dot(d, U) / (tt * dot(U, U));
            px = ((ca + 1.0f) * 0.5f) * (float)W;
            pr = (float)(H - 1) - ((1.0f - cb) * 0.5f) * (float)H;
            if (in && (pm_f2u(px) != pm_f2u(a) || pm_f2u(pr) != pm_f2u(b))) __builtin_trap();
        }
        cont[2 * i] = px; cont[2 * i + 1] = pr;
    }
}
/* the surface points of a Visibility buffer (0 where not shaded), for the same test */
extern "C" void tr_surface_points(int n, const Tri* tris, const Vis* vis, const float* eye3, float* points, uint8_t* is_shaded)
{
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
    for (int i = 0; i < n; ++i)
    {
        points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = 0.0f;
        is_shaded[i] = shaded(tris, vis[i]) ? 1 : 0;
        if (!is_shaded[i]) continue;
        f3 p, nn;
        surface(tris, vis[i], eye, p, nn);
        points[3 * i] = p.x; points[3 * i + 1] = p.y; points[3 * i + 2] = p.z;
    }
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="temporal_reproject_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.tr_temporal.argtypes = [ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.tr_temporal.restype = None
        L.tr_project.argtypes = [ci, vp, vp, ci, ci, vp, vp]
        L.tr_project.restype = None
        L.tr_surface_points.argtypes = [ci, vp, vp, vp, vp, vp]
        L.tr_surface_points.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rg9(rg):
    """a RayGenerator as 9 float32 {origin, right, up}: an oracle RAYGEN record, or anything of 9 numbers (NaN included)"""
    a = np.ascontiguousarray(rg)
    if a.dtype.names:
        a = a.view(np.float32)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    assert a.size == 9
    return a


def temporal(W, H, frame, tris, vis_cur, vis_prev, eye, rg_prev, rg_cur, opt, hist, res, mode=REPROJECT):
    """One temporal_resampling: merges hist into res IN PLACE (as the reference's kernel does) and returns (res, diag). tris / vis_* /
    opt / hist / res: the oracle's TRIANGLE / VISIBILITY / OPTIONS / RESERVOIR arrays; eye: the current camera's; vis_prev: the
    Visibility buffer of the frame that wrote hist (its shaded pixels are the ones that hold a history)."""
    tris, vis_cur, vis_prev, hist = (np.ascontiguousarray(a) for a in (tris, vis_cur, vis_prev, hist))
    assert tris.dtype.itemsize == 60 and vis_cur.dtype.itemsize == 16 and vis_prev.dtype.itemsize == 16
    assert hist.dtype.itemsize == 76 and res.dtype.itemsize == 76 and res.flags["C_CONTIGUOUS"]
    assert len(hist) == len(res) == len(vis_cur) == len(vis_prev) == W * H
    assert hist.ctypes.data != res.ctypes.data, "the history is read while the result is written"
    diag = np.zeros((W * H, 4), dtype=np.int32)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    a, b = _rg9(rg_prev), _rg9(rg_cur)
    lib().tr_temporal(W, H, int(frame), _p(tris), len(tris), _p(vis_cur), _p(vis_prev), _p(e), _p(a), _p(b), int(opt["ris_sample_count"][0]),
                      int(opt["use_temporal_resampling"][0]), int(opt["use_shadowed_target_function"][0]), int(opt["use_visibility_reuse"][0]),
                      int(mode), _p(hist), _p(res), _p(diag))
    return res, diag


def project(points, rg_prev, W, H):
    """tr_previous_pixel of csrc/temporal_reproject.h for n points: (pix (n, 3) int32 {valid, xq, rq}, cont (n, 2) float32 continuous
    storage coordinates (px, pr), NaN behind the camera)"""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    pix, cont = np.zeros((len(pts), 3), np.int32), np.zeros((len(pts), 2), np.float32)
    a = _rg9(rg_prev)
    lib().tr_project(len(pts), _p(pts), _p(a), W, H, _p(pix), _p(cont))
    return pix, cont


def surface_points(tris, vis, eye):
    """(points (n, 3) float32, shaded (n,) bool) of a Visibility buffer: common/core.hpp:189-207 in binary32, as the G-buffer holds them"""
    tris, vis = np.ascontiguousarray(tris), np.ascontiguousarray(vis)
    pts, sh = np.zeros((len(vis), 3), np.float32), np.zeros(len(vis), np.uint8)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    lib().tr_surface_points(len(vis), _p(tris), _p(vis), _p(e), _p(pts), _p(sh))
    return pts, sh.astype(bool)
