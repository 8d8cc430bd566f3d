"""CPU restatement of generate_candidate (10_restir_di.cu:36-135) with the light selection of rt_light_sampling (csrc/light_alias.h,
DESIGN.md section 12), for tests/test_light_sampling_cpu.py and tests/test_gpu_light_sampling.py.

Plain C++ on the reference's PODs (buffer index = row * W + x). Every formula comes from csrc/rt_device.h and csrc/light_alias.h, the
headers the kernel and the library's host code are compiled from; built with `g++ -ffp-contract=off`, so the records equal the GPU's
bit for bit. mode = UNIFORM draws rv0, bx, by, u per candidate and is the reference's kernel (anchored to
oracle.Scene.generate_candidate by the CPU tests); mode = POWER draws rv0, ra, bx, by, u, takes the light from light_select and divides
by the pdf the table realises. Shadow rays are brute-force any-hit over all triangles, as in tests/restir_unbiased_ref.py.
The module also exports the table builder, its quantisation and light_select."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

UNIFORM, POWER = 0, 1
ONE = 1 << 23

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "rt_device.h"
#include "light_alias.h"
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
static void put(float* a, f3 v) { a[0] = v.x; a[1] = v.y; a[2] = v.z; }
static bool emissive(const Tri& t) { return t.emissive[0] > 0.0f || t.emissive[1] > 0.0f || t.emissive[2] > 0.0f; }
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

/* light list in index order (10_restir_di.cpp:196-205) and the weights of light_alias.h */
extern "C" int ls_lights(const Tri* tris, int n_tris, uint32_t* ids, float* w)
{
    int L = 0;
    for (int i = 0; i < n_tris; ++i)
        if (emissive(tris[i]))
        {
            if (ids) ids[L] = (uint32_t)i;
            if (w) w[L] = light_weight(v3(tris[i].v), v3(tris[i].v + 3), v3(tris[i].v + 6), v3(tris[i].emissive));
            ++L;
        }
    return L;
}
/* q per light (returns T as two halves through T2), then the table; returns 1 if some light has q > 0 */
extern "C" int ls_table(const float* w, uint32_t L, uint64_t* q, uint64_t* T, uint32_t* thr, uint32_t* alias, uint64_t* K)
{
    std::vector<uint64_t> qv, Kv;
    std::vector<AliasSlot> tab;
    *T = alias_quantise(w, L, qv);
    const bool ok = alias_build(w, L, tab, Kv);
    for (uint32_t i = 0; i < L; ++i) { q[i] = qv[i]; thr[i] = tab[i].thr; alias[i] = tab[i].alias; K[i] = Kv[i]; }
    return ok ? 1 : 0;
}
extern "C" uint32_t ls_select(const uint32_t* thr, const uint32_t* alias, uint32_t L, float rv0, float ra)
{
    std::vector<AliasSlot> tab(L);
    for (uint32_t i = 0; i < L; ++i) tab[i] = AliasSlot{thr[i], alias[i]};
    return light_select(tab.data(), L, rv0, ra);
}
/* light_select over all 2^23 values PCG::uniformf can give ra, at the slot rv0 names: counts[light] += 1; returns the slot */
extern "C" uint32_t ls_select_all(const uint32_t* thr, const uint32_t* alias, uint32_t L, float rv0, uint64_t* counts)
{
    std::vector<AliasSlot> tab(L);
    for (uint32_t i = 0; i < L; ++i) tab[i] = AliasSlot{thr[i], alias[i]};
    for (uint32_t k = 0; k < (1u << 23); ++k)
    {
        const float ra = pm_u2f(k | 0x3f800000u) - 1.0f; /* PCG::uniformf */
        counts[light_select(tab.data(), L, rv0, ra)] += 1u;
    }
    return light_slot(L, rv0);
}

extern "C" int ls_generate(int W, int H, int frame, const Tri* tris, int n_tris, const Vis* vis, const float* eye3, int ris_sample_count,
                           int shadowed, int vis_reuse, int mode, Reservoir* out)
{
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]);
    std::vector<uint32_t> ids((size_t)n_tris + 1);
    std::vector<float> w((size_t)n_tris + 1);
    const uint32_t L = (uint32_t)ls_lights(tris, n_tris, ids.data(), w.data());
    std::vector<AliasSlot> tab;
    std::vector<uint64_t> K;
    if (mode == 1 && !alias_build(w.data(), L, tab, K) && ris_sample_count > 0) return 1;
    if (L == 0 && ris_sample_count > 0) return 1;
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
            PCG rng = pcg_init(hashPCG4((uint32_t)xi, (uint32_t)yi, (uint32_t)frame, 0u), 0);
            for (int i = 0; i < ris_sample_count; ++i)
            {
                const float rv0 = rng.uniformf();
                uint32_t nth;
                if (mode == 1) { const float ra = rng.uniformf(); nth = light_select(tab.data(), L, rv0, ra); }
                else nth = light_slot(L, rv0);
                float bx = rng.uniformf();
                float by = rng.uniformf();
                const Tri& lt = tris[ids[nth]];
                const f3 v0 = v3(lt.v), v1 = v3(lt.v + 3), v2 = v3(lt.v + 6);
                warp_unit_triangle(bx, by);
                const f3 lp = (1.0f - bx - by) * v0 + bx * v1 + by * v2;
                const f3 ln = tri_normal(v0, v1, v2);
                const float sel = mode == 1 ? light_select_prob(K[nth], L) : 1.0f / (float)(size_t)L;
                const float pdf = sel * 1.0f / tri_area(v0, v1, v2);
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
        d = tempfile.mkdtemp(prefix="light_sampling_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                               "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci, u32, f = C.c_void_p, C.c_int, C.c_uint32, C.c_float
        L.ls_lights.argtypes = [vp, ci, vp, vp]
        L.ls_table.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.ls_select.argtypes = [vp, vp, u32, f, f]
        L.ls_select.restype = u32
        L.ls_select_all.argtypes = [vp, vp, u32, f, vp]
        L.ls_select_all.restype = u32
        L.ls_generate.argtypes = [ci, ci, ci, vp, ci, vp, vp, ci, ci, ci, ci, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lights(tris):
    """(ids, weights) of the emissive triangles in index order"""
    tris = np.ascontiguousarray(tris)
    assert tris.dtype.itemsize == 60
    ids, w = np.zeros(len(tris) + 1, np.uint32), np.zeros(len(tris) + 1, np.float32)
    n = lib().ls_lights(_p(tris), len(tris), _p(ids), _p(w))
    return ids[:n].copy(), w[:n].copy()


def table(w):
    """the alias table of the weights w: dict(ok, q, T, thr, alias, K)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    n = len(w)
    q, K, T = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(1, np.uint64)
    thr, alias = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ok = lib().ls_table(_p(w), n, _p(q), _p(T), _p(thr), _p(alias), _p(K))
    return dict(ok=bool(ok), q=q, T=int(T[0]), thr=thr, alias=alias, K=K)


def select(t, rv0, ra):
    return int(lib().ls_select(_p(t["thr"]), _p(t["alias"]), len(t["thr"]), C.c_float(rv0), C.c_float(ra)))


def select_all(t, rv0):
    """(slot of rv0, how often light_select names each light over the 2^23 values of ra)"""
    counts = np.zeros(len(t["thr"]), np.uint64)
    slot = lib().ls_select_all(_p(t["thr"]), _p(t["alias"]), len(t["thr"]), C.c_float(rv0), _p(counts))
    return int(slot), counts


def generate_candidate(W, H, frame, tris, vis, eye, opt, mode, res=None):
    """generate_candidate over the whole image. tris / vis / opt: the oracle's TRIANGLE / VISIBILITY / OPTIONS arrays; res: RESERVOIR
    array to fill (every pixel is written, as the reference does). Raises where the library returns RT_ERR_STATE."""
    tris, vis = np.ascontiguousarray(tris), np.ascontiguousarray(vis)
    assert tris.dtype.itemsize == 60 and vis.dtype.itemsize == 16 and len(vis) == W * H
    if res is None:
        from oracle import binding as ob

        res = np.zeros(W * H, dtype=ob.RESERVOIR)
    assert res.dtype.itemsize == 76 and len(res) == W * H and res.flags.c_contiguous
    e = np.ascontiguousarray(eye, dtype=np.float32)
    rc = lib().ls_generate(W, H, int(frame), _p(tris), len(tris), _p(vis), _p(e), int(opt["ris_sample_count"][0]),
                           int(opt["use_shadowed_target_function"][0]), int(opt["use_visibility_reuse"][0]), int(mode), _p(res))
    if rc:
        raise RuntimeError("no light can be selected")
    return res


LAMP_EYE, LAMP_AT = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5)


def make_lamp_room(triangle_dtype=None):
    """make_quad_room's floor, wall and box under one bright 2 x 2 panel (Ke = 20) and 40 dim tiles of 0.05 x 0.05 (Ke between 1 and 5,
    from a seeded LCG): the panel carries 99.6 % of the power and is 2 of the 82 lights, so uniform selection spends 2.4 % of its
    candidates on it. 132 triangles; view: LAMP_EYE -> LAMP_AT."""
    from cedec_2024_rt_amd import scenes

    base = scenes.make_quad_room(n_lights=0)
    rng = scenes._LCG(21)
    quads = [([(-1.0, 5.0, -2.0), (1.0, 5.0, -2.0), (1.0, 5.0, 0.0), (-1.0, 5.0, 0.0)], 20.0)]
    for _ in range(40):
        x = -3.5 + 7.0 * rng.below(1024) / 1024.0
        y = 2.5 + 2.0 * rng.below(1024) / 1024.0
        z = -3.5 + 6.0 * rng.below(1024) / 1024.0
        ke = 1.0 + 4.0 * rng.below(1024) / 1024.0
        quads.append(([(x, y, z), (x + 0.05, y, z), (x + 0.05, y, z + 0.05), (x, y, z + 0.05)], ke))
    t = np.zeros(len(base) + 2 * len(quads), dtype=triangle_dtype or base.dtype)
    for f in ("v", "color", "emissive"):
        t[f][:len(base)] = base[f]
    for i, (q, ke) in enumerate(quads):
        q = np.array(q, np.float32)
        k = len(base) + 2 * i
        t["v"][k], t["v"][k + 1] = q[[0, 1, 2]], q[[0, 2, 3]]
        t["color"][k:k + 2], t["emissive"][k:k + 2] = 0.8, np.float32(ke)
    return t
