"""CPU restatement of the temporal merge with a history that follows moved geometry (rt_temporal_motion; csrc/temporal_motion.h,
csrc/frame_kernels.h: load_prev_motion + temporal_merge_at) for tests/test_temporal_motion_cpu.py and
tests/test_gpu_temporal_motion.py, after the pattern of tests/temporal_reproject_ref.py.

One temporal_resampling over the whole image in plain C++ on the reference's 76-byte Reservoir records (buffer index = row * W + x).
Every formula comes from csrc/rt_device.h, csrc/portable_math.h, csrc/temporal_reproject.h and csrc/temporal_motion.h, the headers the
kernels are compiled from; built with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit. Shadow rays are brute force
over all CURRENT triangles.

tris / vis_cur / eye / rg_cur describe the frame being merged; tris_prev / vis_prev / eye_prev / rg_prev the frame that wrote the
history; [lo, hi) is the moved range. A shaded pixel whose triangle lies outside the range takes the own pixel's record where the 36
bytes of the two RayGenerators are equal and the record of temporal_reproject_ref otherwise, and its rejection heuristics are the
reference's. A shaded pixel on a triangle inside the range interpolates its (u, v) over tris_prev, projects that point into rg_prev
(equal bytes or not), takes the nearest pixel's record where that pixel was shaded in the previous frame, Reservoir{} otherwise, and
evaluates the heuristics on the previous point, its normal and eye_prev. diag holds per pixel {valid, xq, rq, in_range}: in_range =
the pixel lies on a triangle of the range; valid = a history was gathered for it through a projection (0 for the own-pixel path);
(xq, rq) = the projected pixel, 0 where none. Pixels that are not shaded: {0, 0, 0, 0}."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from temporal_reproject_ref import _p, _rg9

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "rt_device.h"
#include "temporal_motion.h"
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


static Reservoir gather(const Tri* tris_prev, const Vis* vis_prev, const Reservoir* hist, int W, int H, const TrPixel t, int32_t* D)
{
    Reservoir pr;
    memset(&pr, 0, sizeof(pr));
    if (t.valid)
    {
        /* the index exists only behind the range test; the restatement aborts rather than read outside its buffers */
        const size_t qi = (size_t)t.xq + (size_t)t.rq * W;
        if (t.xq < 0 || t.xq >= W || t.rq < 0 || t.rq >= H || qi >= (size_t)W * (size_t)H) __builtin_trap();
        D[1] = t.xq; D[2] = t.rq;
        if (shaded(tris_prev, vis_prev[qi])) { pr = hist[qi]; D[0] = 1; }
    }
    return pr;
}

extern "C" void tm_temporal(int W, int H, int frame, const Tri* tris, const Tri* tris_prev, int n_tris, const Vis* vis_cur, const Vis* vis_prev,
                            const float* eye3, const float* eye_prev3, const float* rg_prev, const float* rg_cur, uint32_t lo, uint32_t hi,
                            int ris_sample_count, int use_temporal, int shadowed, int vis_reuse, const Reservoir* hist, Reservoir* res, int32_t* diag)
{
    const f3 eye = v3(eye3), eye_prev = v3(eye_prev3);
    const bool same_camera = tr_same_camera(rg_prev, rg_cur);
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
            Reservoir r = res[q];
            Reservoir pr;
            f3 h_p = v3(r.origin_position), h_n = v3(r.origin_normal), h_eye = eye;
            if (tm_in_range(vis_cur[q].index, lo, hi))
            {
                D[3] = 1;
                const Tri& t = tris_prev[vis_cur[q].index];
                const TmSurface s = tm_previous_surface(v3(t.v), v3(t.v + 3), v3(t.v + 6), vis_cur[q].u, vis_cur[q].v, eye_prev);
                pr = gather(tris_prev, vis_prev, hist, W, H, tr_previous_pixel(s.p, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H), D);
                h_p = s.p; h_n = s.n; h_eye = eye_prev;
            }
            else if (same_camera) pr = hist[q];
            else pr = gather(tris_prev, vis_prev, hist, W, H, tr_previous_pixel(sp, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H), D);
            const int cap = 20 * ris_sample_count;
            pr.M = pr.M < cap ? pr.M : cap;
            float p_hat_y = target(tris, n_tris, sp, sn, pr, shadowed);
            if (vis_reuse) p_hat_y *= pr.visibility ? 1.0f : 0.0f;
            pr.M = scale_M(pr.M, rejection_heuristics(h_p, h_n, v3(pr.origin_position), v3(pr.origin_normal), h_eye));
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

/* the previous surface points and normals of a Visibility buffer's pixels on triangles of [lo, hi) (0 and in_range = 0 elsewhere), for
 * the test of the lookup against the float64 statement */
extern "C" void tm_previous_points(int n, const Tri* tris, const Tri* tris_prev, const Vis* vis, const float* eye_prev3, uint32_t lo, uint32_t hi,
                                   float* points, float* normals, uint8_t* in_range)
{
    for (int i = 0; i < n; ++i)
    {
        points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = 0.0f;
        normals[3 * i] = normals[3 * i + 1] = normals[3 * i + 2] = 0.0f;
        in_range[i] = shaded(tris, vis[i]) && tm_in_range(vis[i].index, lo, hi) ? 1 : 0;
        if (!in_range[i]) continue;
        const Tri& t = tris_prev[vis[i].index];
        const TmSurface s = tm_previous_surface(v3(t.v), v3(t.v + 3), v3(t.v + 6), vis[i].u, vis[i].v, v3(eye_prev3));
        points[3 * i] = s.p.x; points[3 * i + 1] = s.p.y; points[3 * i + 2] = s.p.z;
        normals[3 * i] = s.n.x; normals[3 * i + 1] = s.n.y; normals[3 * i + 2] = s.n.z;
    }
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="temporal_motion_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci, cu = C.c_void_p, C.c_int, C.c_uint32
        L.tm_temporal.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, cu, cu, ci, ci, ci, ci, vp, vp, vp]
        L.tm_temporal.restype = None
        L.tm_previous_points.argtypes = [ci, vp, vp, vp, vp, cu, cu, vp, vp, vp]
        L.tm_previous_points.restype = None
        _lib = L
    return _lib


def temporal(W, H, frame, tris, tris_prev, vis_cur, vis_prev, eye, eye_prev, rg_prev, rg_cur, lo, hi, opt, hist, res):
    """One temporal_resampling: merges hist into res IN PLACE and returns (res, diag). tris / tris_prev: the oracle's TRIANGLE arrays of
    the current frame and of the frame that wrote hist (same count and order); vis_* / opt / hist / res: its VISIBILITY / OPTIONS /
    RESERVOIR arrays; [lo, hi): the moved range."""
    tris, tris_prev, vis_cur, vis_prev, hist = (np.ascontiguousarray(a) for a in (tris, tris_prev, vis_cur, vis_prev, hist))
    assert tris.dtype.itemsize == 60 and tris_prev.dtype.itemsize == 60 and len(tris) == len(tris_prev)
    assert vis_cur.dtype.itemsize == 16 and vis_prev.dtype.itemsize == 16
    assert hist.dtype.itemsize == 76 and res.dtype.itemsize == 76 and res.flags["C_CONTIGUOUS"]
    assert len(hist) == len(res) == len(vis_cur) == len(vis_prev) == W * H
    assert hist.ctypes.data != res.ctypes.data, "the history is read while the result is written"
    assert 0 <= lo <= hi <= len(tris)
    diag = np.zeros((W * H, 4), dtype=np.int32)
    e, ep = np.ascontiguousarray(eye, dtype=np.float32), np.ascontiguousarray(eye_prev, dtype=np.float32)
    a, b = _rg9(rg_prev), _rg9(rg_cur)
    lib().tm_temporal(W, H, int(frame), _p(tris), _p(tris_prev), len(tris), _p(vis_cur), _p(vis_prev), _p(e), _p(ep), _p(a), _p(b), int(lo), int(hi),
                      int(opt["ris_sample_count"][0]), int(opt["use_temporal_resampling"][0]), int(opt["use_shadowed_target_function"][0]),
                      int(opt["use_visibility_reuse"][0]), _p(hist), _p(res), _p(diag))
    return res, diag


def previous_points(tris, tris_prev, vis, eye_prev, lo, hi):
    """(points (n, 3) float32, normals (n, 3) float32, in_range (n,) bool): tm_previous_surface of csrc/temporal_motion.h for the shaded pixels of `vis` that lie on
    triangles of [lo, hi), in binary32 as the kernels compute it"""
    tris, tris_prev, vis = (np.ascontiguousarray(a) for a in (tris, tris_prev, vis))
    pts, nrm, m = np.zeros((len(vis), 3), np.float32), np.zeros((len(vis), 3), np.float32), np.zeros(len(vis), np.uint8)
    e = np.ascontiguousarray(eye_prev, dtype=np.float32)
    lib().tm_previous_points(len(vis), _p(tris), _p(tris_prev), _p(vis), _p(e), int(lo), int(hi), _p(pts), _p(nrm), _p(m))
    return pts, nrm, m.astype(bool)
