"""CPU restatement of the indirect pass (rt_indirect; csrc/indirect.h, csrc/frame_kernels.h k_indirect) for
tests/test_indirect_cpu.py and tests/test_gpu_indirect.py.

One pass over the whole image in plain C++ (buffer index = row * W + x). The start of a path (indirect_start), sample_hemisphere and
bounce_direction come from csrc/indirect.h, the header the kernels are compiled from. The depth loop is stated here on its own, after
the oracle's 08_nee (light point, pdf 1 / n_lights / area, next-event term), with the small functions of csrc/rt_device.h and
csrc/portable_math.h: the kernels run path_bounce<8, false> with the light table's stored pdf instead, which tests/test_gpu_parity.py
holds to the oracle bit for bit. Built with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit (rows run on OpenMP threads:
a pixel is computed by one thread). The closest hit is brute force over all triangles under the parity contract's definition
(common/core.hpp:91-136 over [tmin, best], so that of equal distances the highest index stands), the shadow ray
brute-force any-hit: the BVH walks equal brute force (csrc/bvh_cull.h has the argument, tests/test_gpu_targeted_rays.py the rays).

Two starts behind a switch. GBUFFER is the product's: the surface comes from the Visibility record through make_surface_info's
arithmetic (common/core.hpp:189-207), as the raycast kernel fills g0 / g1. CAMERA is 08_nee's own: the primary ray, sp = ro + t rd, the
normal flipped by the ray; with it  oracle path_trace(8, max_depth = 1) + tail(bounces = D - 1)  is  oracle path_trace(8, max_depth = D)
up to the grouping of the sum, which anchors the restatement to the oracle."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

GBUFFER, CAMERA = 0, 1

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <vector>
#include "indirect.h"
using namespace rt;

struct Tri { float v[9], color[3], emissive[3]; };
struct Vis { float u, v; int32_t index, pad; };
static_assert(sizeof(Tri) == 60 && sizeof(Vis) == 16, "the reference's PODs");

static f3 v3(const float* a) { return F3(a[0], a[1], a[2]); }
static bool emissive(const Tri& t) { return t.emissive[0] > 0.0f || t.emissive[1] > 0.0f || t.emissive[2] > 0.0f; }
/* the pinned definition of raytrace() (common/raytrace.hpp:18-43) */
static int closest_hit(const Tri* tris, int n_tris, f3 ro, f3 rd, float& t_out)
{
    float best = kFltMax;
    int index = -1;
    for (int i = 0; i < n_tris; ++i)
    {
        float t, u, v;
        if (intersect_ray_triangle(t, u, v, ro, rd, 0.0f, best, v3(tris[i].v), v3(tris[i].v + 3), v3(tris[i].v + 6))) { best = t; index = i; }
    }
    t_out = best;
    return index;
}
/* common/raytrace.hpp:45-52 */
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

/* 08_nee.cu:66-69: the light point of the draws (bx, by) on the emissive triangle (a0, a1, a2) */
static f3 nee_light_point(f3 a0, f3 a1, f3 a2, float bx, float by)
{
    warp_unit_triangle(bx, by);
    return (1.0f - bx - by) * a0 + bx * a1 + by * a2;
}
/* 08_nee.cu:84-87: pdf of a uniformly picked light, uniformly sampled over its area */
static float nee_light_pdf(int n_lights, float area) { return 1.0f / (float)(size_t)n_lights * 1.0f / area; }
/* 08_nee.cu:89-90: ((((throughput * brdf) * G) * V) * Le) / pdf */
static f3 nee_term(f3 throughput, f3 kd, float G, float V, f3 ke, float pdf)
{
    const f3 brdf = (1.0f / kPI) * kd;
    return throughput * brdf * G * V * ke / pdf;
}

/* accum: W * H x {r, g, b, n}: the pass ADDS to r, g, b and leaves n. stats: {paths started, raytrace() calls, paths alive when the
 * last bounce started}. rg9: the RayGenerator's origin, right, up (CAMERA start), eye3: the eye (GBUFFER start). */
extern "C" void ind_pass(int W, int H, int frame, const Tri* tris, int n_tris, const Vis* vis, const float* eye3, const float* rg9, int start,
                         int bounces, float* accum, uint64_t* stats)
{
    const f3 eye = v3(eye3), origin = v3(rg9), right = v3(rg9 + 3), up = v3(rg9 + 6);
    std::vector<int> lights;
    for (int i = 0; i < n_tris; ++i)
        if (emissive(tris[i])) lights.push_back(i);
    const int n_lights = (int)lights.size();
    long long paths = 0, rays = 0, alive_last = 0;
    if (bounces < 1 || n_lights == 0) { stats[0] = stats[1] = stats[2] = 0; return; }
#pragma omp parallel for schedule(dynamic, 2) reduction(+ : paths, rays, alive_last)
    for (int row = 0; row < H; ++row)
        for (int xi = 0; xi < W; ++xi)
        {
            const int yi = H - 1 - row;
            const size_t q = (size_t)xi + (size_t)row * W;
            int tri;
            f3 sp, sn;
            if (start == 0)
            {
                /* common/core.hpp:189-207 on the Visibility record (frame_kernels.h, surface_info) */
                tri = vis[q].index;
                if (tri < 0 || emissive(tris[tri])) continue;
                const f3 v0 = v3(tris[tri].v), v1 = v3(tris[tri].v + 3), v2 = v3(tris[tri].v + 6);
                sp = (1.0f - vis[q].u - vis[q].v) * v0 + vis[q].u * v1 + vis[q].v * v2;
                sn = tri_normal(v0, v1, v2);
                if (dot(normalize(eye - sp), sn) < 0.0f) sn = -sn;
            }
            else
            {
                /* common/camera.hpp:27-35 shoot(xi / W, yi / H), then 08_nee.cu:41-64 at depth 0 */
                const float u = (float)xi / (float)W, v = (float)yi / (float)H;
                const f3 forward = normalize(cross(up, right));
                const f3 to = origin + forward + mix(-right, right, u) + mix(up, -up, v);
                const f3 rd = normalize(to - origin);
                float t;
                tri = closest_hit(tris, n_tris, origin, rd, t);
                if (tri < 0 || emissive(tris[tri])) continue;
                sp = origin + t * rd;
                sn = tri_normal(v3(tris[tri].v), v3(tris[tri].v + 3), v3(tris[tri].v + 6));
                if (dot(-rd, sn) < 0.0f) sn = -sn;
            }
            ++paths;
            const IndirectStart s = indirect_start(xi, yi, frame, sp, sn, v3(tris[tri].color), v3(tris[tri].v), v3(tris[tri].v + 3));
            f3 ro = s.ro, rd = s.rd, throughput = s.throughput, radiance = F3(0.0f, 0.0f, 0.0f);
            PCG rng = s.rng;
            for (int depth = 1; depth <= bounces; ++depth)
            {
                if (depth == bounces) ++alive_last;
                /* 08_nee.cu:39-118 at depth >= 1 */
                float t;
                ++rays;
                const int h = closest_hit(tris, n_tris, ro, rd, t);
                if (h < 0) break;            /* the sky is not a light */
                if (emissive(tris[h])) break; /* emission counts at depth 0 only */
                const f3 v0 = v3(tris[h].v), v1 = v3(tris[h].v + 3), v2 = v3(tris[h].v + 6), kd = v3(tris[h].color);
                const f3 p = ro + t * rd;
                f3 n = tri_normal(v0, v1, v2);
                if (dot(-rd, n) < 0.0f) n = -n;
                const float rv0 = rng.uniformf();
                const float bx = rng.uniformf();
                const float by = rng.uniformf();
                uint32_t nth = (uint32_t)(rv0 * (float)(size_t)n_lights);
                if (nth == (uint32_t)n_lights) nth = (uint32_t)n_lights - 1u;
                const Tri& lt = tris[lights[nth]];
                const f3 a0 = v3(lt.v), a1 = v3(lt.v + 3), a2 = v3(lt.v + 6);
                const f3 lp = nee_light_point(a0, a1, a2, bx, by);
                const f3 ln = tri_normal(a0, a1, a2);
                const float V = check_visibility(tris, n_tris, p, n, lp) ? 1.0f : 0.0f;
                ++rays;
                const float G = geometry_term(p, n, lp, ln);
                radiance = radiance + nee_term(throughput, kd, G, V, v3(lt.emissive), nee_light_pdf(n_lights, tri_area(a0, a1, a2)));
                const float r0 = rng.uniformf();
                const float r1 = rng.uniformf();
                const float r2 = rng.uniformf();
                rd = bounce_direction(v0, v1, n, sample_hemisphere(r0, r1, r2));
                throughput = throughput * kd;
                ro = p + 0.001f * n;
            }
            float* a = accum + 4 * q;
            a[0] = a[0] + radiance.x; a[1] = a[1] + radiance.y; a[2] = a[2] + radiance.z;
        }
    stats[0] = (uint64_t)paths; stats[1] = (uint64_t)rays; stats[2] = (uint64_t)alive_last;
}
"""

_lib = None


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="indirect_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.ind_pass.argtypes = [ci, ci, ci, vp, ci, vp, vp, vp, ci, ci, vp, vp]
        L.ind_pass.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def add(accum, W, H, frame, tris, vis, eye, raygen, bounces, start=GBUFFER):
    """The pass on top of `accum` ((W * H, 4) float32, changed in place: RGB added, .w left). tris / vis / raygen: the oracle's
    TRIANGLE / VISIBILITY / RAYGEN arrays. Returns dict(paths, rays, alive_last) as rt_indirect_stats reports them."""
    tris, vis = np.ascontiguousarray(tris), np.ascontiguousarray(vis)
    assert tris.dtype.itemsize == 60 and vis.dtype.itemsize == 16 and len(vis) == W * H
    assert accum.dtype == np.float32 and accum.flags.c_contiguous and accum.size == 4 * W * H
    e = np.ascontiguousarray(eye, dtype=np.float32)
    rg = np.ascontiguousarray(raygen).view(np.float32).reshape(-1)[:9].copy()
    st = np.zeros(3, np.uint64)
    lib().ind_pass(W, H, int(frame), _p(tris), len(tris), _p(vis), _p(e), _p(rg), int(start), int(bounces), _p(accum), _p(st))
    return dict(paths=int(st[0]), rays=int(st[1]), alive_last=int(st[2]))


def tail(W, H, frame, tris, vis, eye, raygen, bounces, start=GBUFFER):
    """the pass on a zeroed buffer: ((W * H, 3) float32 radiance of the tail, stats)"""
    acc = np.zeros((W * H, 4), np.float32)
    st = add(acc, W, H, frame, tris, vis, eye, raygen, bounces, start)
    assert not acc[:, 3].any()
    return acc[:, :3].copy(), st
