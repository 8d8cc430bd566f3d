"""CPU restatement of the temporal merge with the 1/Z normalisation (rt_temporal_unbiased; csrc/temporal_unbiased.h,
csrc/frame_kernels.h: k_temporal_unbiased) for tests/test_temporal_unbiased_cpu.py and
tests/test_gpu_temporal_unbiased.py.

One temporal_resampling over the whole image in plain C++ on the reference's 76-byte Reservoir records (buffer index = row * W + x),
in the style of tests/temporal_reproject_ref.py. The estimator is compiled from csrc/temporal_unbiased.h, the header the kernel is
compiled from, with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit. Shadow rays are brute force over all
triangles with intersect_ray_triangle (the BVH walk equals brute force: csrc/bvh_cull.h).
mode = REFERENCE / REPROJECT are temporal_reproject_ref's two modes, restated here bit for bit (the switch off). mode = UNBIASED is
the toggle on: with the 36 bytes of the two RayGenerators equal it is the reference's merge (the host launches the same kernels),
with other bytes every shaded pixel merges the history load_prev_reprojected gives it by the 1/Z estimator.
diag holds per pixel {valid, from_hist, in_Z, ray}: valid = a history was merged (REFERENCE: the own pixel's, always; otherwise the
gathered pixel was shaded in the previous Visibility buffer), from_hist = the history's sample was selected, in_Z = the history's M
counts in the normalisation (REFERENCE / REPROJECT: whenever valid, that is the 1/M merge; UNBIASED: Mk > 0 and the selected sample
lies in the history's support), ray = a shadow ray was walked from the history's origin. Pixels that are not shaded: {0, 0, 0, 0}.
A fifth and sixth column hold Mk (the history's M after the cap and the rejection heuristics) and Z."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

REFERENCE, REPROJECT, UNBIASED = 0, 1, 2
DIAG_COLS = 6

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "rt_device.h"
#include "temporal_reproject.h"
#include "temporal_unbiased.h"
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
/* the record type temporal_unbiased.h's templates work on */
struct Rec { f3 hit_p, hit_n, org_p, org_n; float lum, ucw, w_sum; int M; bool vis; };

static f3 v3(const float* a) { return F3(a[0], a[1], a[2]); }
static void put(float* a, f3 v) { a[0] = v.x; a[1] = v.y; a[2] = v.z; }
static Rec rec_of(const Reservoir& r)
{
    Rec o;
    o.hit_p = v3(r.hit_position); o.hit_n = v3(r.hit_normal); o.org_p = v3(r.origin_position); o.org_n = v3(r.origin_normal);
    o.lum = luminance(v3(r.radiance)); o.ucw = r.ucw; o.w_sum = r.w_sum; o.M = r.M; o.vis = r.visibility != 0;
    return o;
}
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
static bool visible(const Tri* tris, int n_tris, f3 p0, f3 n0, f3 p1)
{
    const f3 org = p0 + 0.001f * n0, dir = p1 - p0;
    for (int i = 0; i < n_tris; ++i)
    {
        float t, u, v;
        if (intersect_ray_triangle(t, u, v, org, dir, 0.0f, 0.99f, v3(tris[i].v), v3(tris[i].v + 3), v3(tris[i].v + 6))) return false;
    }
    return true;
}
/* common/reservoir.hpp:42-59 */
static float target(const Tri* tris, int n_tris, f3 sp, f3 sn, const Reservoir& r, int shadowed)
{
    const f3 hp = v3(r.hit_position), hn = v3(r.hit_normal);
    const float lum = luminance(v3(r.radiance));
    if (!shadowed) return target_unshadowed(sp, sn, hp, hn, lum);
    return (1.0f / kPI) * geometry_term(sp, sn, hp, hn) * (visible(tris, n_tris, sp, sn, hp) ? 1.0f : 0.0f) * lum;
}

/* rg_prev / rg_cur: 9 floats each {origin, right, up}; diag: 6 ints per pixel, see the module's text. Returns 0, or -1 for what
 * the product refuses (the shadowed target function in an unbiased launch). */
extern "C" int tu_temporal(int W, int H, int frame, const Tri* tris, int n_tris, const Vis* vis_cur, const Vis* vis_prev, const float* eye3,
                           const float* rg_prev, const float* rg_cur, int ris_sample_count, int use_temporal, int shadowed, int vis_reuse, int mode,
                           const Reservoir* hist, Reservoir* res, int32_t* diag)
{
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
    const bool gather = mode >= 1 && !tr_same_camera(rg_prev, rg_cur);
    const bool unbiased = mode == 2 && gather;
    if (unbiased && shadowed && use_temporal) return -1;
    const size_t n_px = (size_t)W * (size_t)H;
#pragma omp parallel for schedule(dynamic, 2)
    for (int row = 0; row < H; ++row)
        for (int xi = 0; xi < W; ++xi)
        {
            const int yi = H - 1 - row;
            const size_t q = (size_t)xi + (size_t)row * W;
            int32_t* D = diag + 6 * q;
            for (int k = 0; k < 6; ++k) D[k] = 0;
            if (!shaded(tris, vis_cur[q])) continue;
            if (!use_temporal) continue;
            f3 sp, sn;
            surface(tris, vis_cur[q], eye, sp, sn);
            PCG rng = pcg_init(hashPCG4((uint32_t)xi, (uint32_t)yi, (uint32_t)frame, 1u), 0);
            Reservoir pr;
            if (!gather) { pr = hist[q]; D[0] = 1; }
            else
            {
                memset(&pr, 0, sizeof(pr));
                const TrPixel t = tr_previous_pixel(sp, v3(rg_prev), v3(rg_prev + 3), v3(rg_prev + 6), W, H);
                if (t.valid)
                {
                    /* the index exists only behind the range test; the restatement aborts rather than read outside its buffers */
                    const size_t qi = (size_t)t.xq + (size_t)t.rq * W;
                    if (t.xq < 0 || t.xq >= W || t.rq < 0 || t.rq >= H || qi >= n_px) __builtin_trap();
                    if (shaded(tris, vis_prev[qi])) { pr = hist[qi]; D[0] = 1; }
                }
            }
            Reservoir r = res[q];
            if (!unbiased)
            {
                /* 10_restir_di.cu:177-233 as tests/temporal_reproject_ref.py states it */
                const int cap = 20 * ris_sample_count;
                pr.M = pr.M < cap ? pr.M : cap;
                float p_hat_y = target(tris, n_tris, sp, sn, pr, shadowed);
                if (vis_reuse) p_hat_y *= pr.visibility ? 1.0f : 0.0f;
                pr.M = scale_M(pr.M, rejection_heuristics(v3(r.origin_position), v3(r.origin_normal), v3(pr.origin_position), v3(pr.origin_normal), eye));
                const float weight = p_hat_y * pr.ucw * (float)pr.M;
                const float u = rng.uniformf();
                const int Z0 = r.M;
                r.w_sum += weight;
                r.M += pr.M;
                if (reservoir_accept(u, weight, r.w_sum))
                {
                    memcpy(r.origin_position, pr.origin_position, 15 * sizeof(float));
                    r.visibility = pr.visibility;
                    memcpy(r.pad, pr.pad, 3);
                    D[1] = 1;
                }
                const float p_hat = target(tris, n_tris, sp, sn, r, shadowed);
                r.ucw = p_hat > 0.0f ? r.w_sum / ((float)r.M * p_hat) : 0.0f;
                D[2] = D[0]; D[4] = pr.M; D[5] = Z0 + pr.M;
                res[q] = r;
                continue;
            }
            /* csrc/temporal_unbiased.h: the two halves with the rays between them */
            Rec a = rec_of(r), b = rec_of(pr);
            const float u = rng.uniformf();
            const TuChain c = tu_merge_chain(a, b, sp, sn, eye, ris_sample_count, vis_reuse != 0, u);
            const bool in_geo = tu_hist_geometry(c, a, b);
            bool hist_visible = true, own_visible = true;
            if (tu_needs_hist_ray(c, in_geo, vis_reuse != 0)) { hist_visible = visible(tris, n_tris, b.org_p, b.org_n, a.hit_p); D[3] = 1; }
            if (tu_needs_own_ray(c, vis_reuse != 0)) own_visible = visible(tris, n_tris, sp, sn, a.hit_p);
            const bool in = tu_finish(a, b, c, in_geo, vis_reuse != 0, hist_visible, own_visible, sp, sn);
            if (c.from_hist)
            {
                /* the sample travels as the reference's struct copy moves it; the origin is overwritten below */
                memcpy(r.origin_position, pr.origin_position, 15 * sizeof(float));
                memcpy(r.pad, pr.pad, 3);
            }
            put(r.origin_position, a.org_p); put(r.origin_normal, a.org_n);
            r.visibility = a.vis ? 1 : 0;
            r.w_sum = a.w_sum; r.ucw = a.ucw; r.M = a.M;
            D[1] = c.from_hist ? 1 : 0; D[2] = in ? 1 : 0; D[4] = c.Mk; D[5] = c.Z + (in ? c.Mk : 0);
            res[q] = r;
        }
    return 0;
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="temporal_unbiased_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.tu_temporal.argtypes = [ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.tu_temporal.restype = ci
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


class Unsupported(Exception):
    """what the product answers RT_ERR_UNSUPPORTED to"""


def temporal(W, H, frame, tris, vis_cur, vis_prev, eye, rg_prev, rg_cur, opt, hist, res, mode=UNBIASED):
    """One temporal_resampling: merges hist into res IN PLACE (as the kernels do) and returns (res, diag). tris / vis_* / opt / hist /
    res: the oracle's TRIANGLE / VISIBILITY / OPTIONS / RESERVOIR arrays; eye: the current camera's; vis_prev: the Visibility buffer
    of the frame that wrote hist (its shaded pixels are the ones that hold a history)."""
    tris, vis_cur, vis_prev, hist = (np.ascontiguousarray(a) for a in (tris, vis_cur, vis_prev, hist))
    assert tris.dtype.itemsize == 60 and vis_cur.dtype.itemsize == 16 and vis_prev.dtype.itemsize == 16
    assert hist.dtype.itemsize == 76 and res.dtype.itemsize == 76 and res.flags["C_CONTIGUOUS"]
    assert len(hist) == len(res) == len(vis_cur) == len(vis_prev) == W * H
    assert hist.ctypes.data != res.ctypes.data, "the history is read while the result is written"
    diag = np.zeros((W * H, DIAG_COLS), dtype=np.int32)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    a, b = _rg9(rg_prev), _rg9(rg_cur)
    rc = lib().tu_temporal(W, H, int(frame), _p(tris), len(tris), _p(vis_cur), _p(vis_prev), _p(e), _p(a), _p(b), int(opt["ris_sample_count"][0]),
                           int(opt["use_temporal_resampling"][0]), int(opt["use_shadowed_target_function"][0]), int(opt["use_visibility_reuse"][0]),
                           int(mode), _p(hist), _p(res), _p(diag))
    if rc != 0:
        raise Unsupported("the shadowed target function in an unbiased launch")
    return res, diag
