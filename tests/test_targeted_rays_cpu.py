"""The cull of the 4-wide walk on the CPU, on rays aimed at vertices, edges, box faces and duplicated triangles
(tests/targeted_rays.py).

1. The reference is anchored: the oracle's own BVH (padded boxes, (plane - ro) * inv) returns its brute force bit for bit on
   every scene and distance, so `Scene.trace_closest(rays, force_brute=True)` is what tests/test_gpu_targeted_rays.py compares
   the device walks with.
2. csrc/bvh_cull.h is RT_HD, so `g++ -ffp-contract=off` compiles the accept predicate hipcc compiles (as
   tests/test_bvh_fragment_cpu.py does for the fragments). Records are built with wide_quant_scale / wide_quant_child from the
   scenes' triangles as the builders build them: leaf boxes grown by the build's pad, four leaf children each, and two-level
   chains of them. Every ray that intersect_ray_triangle (rt_device.h) accepts for a triangle must be accepted by the box of
   the child that holds it, with best = tmax and with best = the hit's own t (the tie rule of duplicated geometry).
3. The walks' expression as it stood before the header existed is kept in the program as a second function: it must agree with
   the header on every ray, and on UNPADDED boxes both must LOSE hits on the floor tiles at dist 3. That is the case the
   argument in bvh_cull.h leans on the pad for; if nothing is lost there, these rays no longer reach the place where a cull goes
   wrong.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import targeted_rays as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "bvh_cull.h"
using namespace rt;

struct Record
{
    float o[3];
    uint32_t ebits, q[6];
};
/* the record the builders write for these child boxes (bvh_build_host.h::collapse_wide) */
static Record make_record(const float (*clo)[3], const float (*chi)[3], int n)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, scale[3];
    for (int k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], clo[k][a]); hi[a] = fmaxf(hi[a], chi[k][a]); }
    Record r = {};
    r.ebits = wide_quant_scale(lo, hi, scale);
    for (int k = 0; k < n; ++k) wide_quant_child(lo, scale, clo[k], chi[k], k, r.q);
    for (int a = 0; a < 3; ++a) r.o[a] = lo[a];
    return r;
}
/* ---- the walks' accept test as it stood in each of them before bvh_cull.h, restated ---- */
static bool accept_parent(const Record& r, const uint32_t* n, const uint32_t* f, f3 ro, f3 inv, float tmin, float best, int k)
{
    const float sx = wide_scale(r.ebits, 0), sy = wide_scale(r.ebits, 1), sz = wide_scale(r.ebits, 2);
    const float Ax = (r.o[0] - ro.x) * inv.x, Ay = (r.o[1] - ro.y) * inv.y, Az = (r.o[2] - ro.z) * inv.z;
    const float Bx = sx * inv.x, By = sy * inv.y, Bz = sz * inv.z;
    float tn = fmaxf(fmaxf(__builtin_fmaf(wide_byte(n[0], k), Bx, Ax), __builtin_fmaf(wide_byte(n[1], k), By, Ay)), __builtin_fmaf(wide_byte(n[2], k), Bz, Az));
    float tf = fminf(fminf(__builtin_fmaf(wide_byte(f[0], k), Bx, Ax), __builtin_fmaf(wide_byte(f[1], k), By, Ay)), __builtin_fmaf(wide_byte(f[2], k), Bz, Az));
    tn = fmaxf(tn, tmin);
    tf = fminf(tf, best) * (1.0f + 0x1p-20f);
    return tn <= tf;
}
/* ---- the header ---- */
static bool accept_header(const Record& r, const uint32_t* n, const uint32_t* f, f3 ro, f3 inv, float tmin, float best, int k)
{
    float tn[4];
    bool h[4];
    wide_accept<4>(r.o[0], r.o[1], r.o[2], r.ebits, n[0], n[1], n[2], f[0], f[1], f[2], ro, inv, tmin, best, tn, h);
    return h[k];
}
/* records over groups of 4 * per_child consecutive triangles (per_child = 1: four leaf children; 4: the parent of four such
 * records, whose child boxes are those records' node boxes), every triangle's box grown by pad. out: 0 hits, 1 / 2 lost by the header with best = tmax / = t,
 * 3 / 4 lost by the restated expression, 5 + kind: hits per target kind, 8 + kind: lost by the restated expression (tmax) */
extern "C" void cull_check(const float* tris, int n_tris, const float* rays, const int* target, const int* kind, int n_rays, int per_child, float pad, long long* out)
{
    const int G = 4 * per_child, n_groups = (n_tris + G - 1) / G;
    std::vector<Record> rec((size_t)n_groups);
    for (int g = 0; g < n_groups; ++g)
    {
        float clo[4][3], chi[4][3];
        int n = 0;
        for (int k = 0; k < 4 && (g * G + k * per_child) < n_tris; ++k, ++n)
        {
            for (int a = 0; a < 3; ++a) { clo[k][a] = INFINITY; chi[k][a] = -INFINITY; }
            for (int j = g * G + k * per_child; j < g * G + (k + 1) * per_child && j < n_tris; ++j)
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a)
                    {
                        clo[k][a] = fminf(clo[k][a], tris[9 * (size_t)j + 3 * c + a] - pad);
                        chi[k][a] = fmaxf(chi[k][a], tris[9 * (size_t)j + 3 * c + a] + pad);
                    }
        }
        rec[(size_t)g] = make_record(clo, chi, n);
    }
    for (int i = 0; i < n_rays; ++i)
    {
        const int j = target[i];
        if (j < 0) continue;
        const float* r = rays + 8 * (size_t)i;
        const float* t9 = tris + 9 * (size_t)j;
        const f3 ro = F3(r[0], r[1], r[2]), rd = F3(r[3], r[4], r[5]);
        float t, u, v;
        if (!intersect_ray_triangle(t, u, v, ro, rd, r[6], r[7], F3(t9[0], t9[1], t9[2]), F3(t9[3], t9[4], t9[5]), F3(t9[6], t9[7], t9[8]))) continue;
        /* as every walk prepares the ray (bvh.h) */
        f3 inv = F3(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        inv.x = fminf(fmaxf(inv.x, -1e30f), 1e30f);
        inv.y = fminf(fmaxf(inv.y, -1e30f), 1e30f);
        inv.z = fminf(fmaxf(inv.z, -1e30f), 1e30f);
        const bool p[3] = {inv.x >= 0.0f, inv.y >= 0.0f, inv.z >= 0.0f};
        const Record& R = rec[(size_t)(j / G)];
        const int k = (j % G) / per_child;
        uint32_t n[3], f[3];
        for (int a = 0; a < 3; ++a) { n[a] = p[a] ? R.q[a] : R.q[3 + a]; f[a] = p[a] ? R.q[3 + a] : R.q[a]; }
        out[0]++;
        out[5 + kind[i]]++;
        if (!accept_header(R, n, f, ro, inv, r[6], r[7], k)) out[1]++;
        if (!accept_header(R, n, f, ro, inv, r[6], t, k)) out[2]++;
        if (!accept_parent(R, n, f, ro, inv, r[6], r[7], k)) { out[3]++; out[8 + kind[i]]++; }
        if (!accept_parent(R, n, f, ro, inv, r[6], t, k)) out[4]++;
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="cull_ref_")
        src, so = os.path.join(d, "cull_ref.cpp"), os.path.join(d, "cull_ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.cull_check.argtypes, L.cull_check.restype = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp], None
        _lib = L
    return _lib


def cull_check(tri_v, rays, tri, kind, per_child, pad=0.0):
    out = np.zeros(11, np.int64)
    tri_v, rays = np.ascontiguousarray(tri_v, np.float32), np.ascontiguousarray(rays, np.float32)
    tri, kind = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(kind, np.int32)
    lib().cull_check(tri_v.ctypes.data, len(tri_v), rays.ctypes.data, tri.ctypes.data, kind.ctypes.data, len(rays), per_child, pad, out.ctypes.data)
    return dict(hits=int(out[0]), lost_tmax=int(out[1]), lost_t=int(out[2]), parent_lost_tmax=int(out[3]), parent_lost_t=int(out[4]),
                hits_by_kind=out[5:8].tolist(), parent_lost_by_kind=out[8:11].tolist())


@pytest.fixture(scope="module")
def portable(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return oracle


@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_oracle_bvh_equals_its_brute_force(portable, name):
    """anchors the reference of the GPU tests: the oracle's BVH == its brute force, bit for bit, on the targeted rays"""
    for dist in T.DISTS:
        rays, _, ref = T.reference(portable, name, dist)
        got = portable.Scene(T.make_tris(T.SCENES[name]), use_bvh=True).trace_closest(rays)
        bad = (got.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
        assert not bad.any(), f"{name} dist {dist}: {int(bad.sum())} of {len(rays)} rays differ"


def build_pad(tri_v):
    """the pad the builders give every leaf box (restir_rt.hip, bvh_refit.h::refit_pad), in binary32"""
    ext = np.float32(np.abs(tri_v).max())
    return float(np.float32(4e-5) * (ext if ext > 1 else np.float32(1.0)))


@pytest.mark.parametrize("per_child", (1, 4), ids=("one_record", "two_levels"))
@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_accept_predicate_keeps_every_hit(name, per_child):
    """whatever intersect_ray_triangle accepts for a triangle, the box of the child that holds it accepts: best = tmax, best = t"""
    v = T.SCENES[name]
    for dist in T.DISTS:
        rays, kind, tri = T.rays_for(name, dist)
        c = cull_check(v, rays[:T.N_RAYS], tri[:T.N_RAYS], kind[:T.N_RAYS], per_child, build_pad(v))
        print(name, dist, per_child, c)
        assert c["hits"] >= 0.4 * T.N_RAYS, c  # the target triangle itself: about half of the vertex and edge targets, minus the range edge
        assert c["lost_tmax"] == 0 and c["lost_t"] == 0, f"{name} dist {dist}: {c}"
        assert (c["parent_lost_tmax"], c["parent_lost_t"]) == (0, 0), f"{name} dist {dist}: the header and the restated expression disagree: {c}"


def test_without_the_pad_the_predicate_loses_hits_on_the_tiles():
    """on UNPADDED boxes the expression loses hits at tile vertices and edges from dist 3, none of them interior (3 826 of
    572 075 when this was found, in a restatement whose decode was not fused; with the FMA the device runs it is 0.11 %). At
    least 1 000 here, over 1.6 million rays; the header and the restated expression lose the same ones; with the build's pad
    (4e-5 * 8) nothing is lost."""
    v = T.SCENES["a_tiles"]
    tot = dict(hits=0, restated=0, header=0, header_t=0, restated_t=0, padded=0, by_kind=np.zeros(3, np.int64))
    for salt in range(8):
        rays, kind, tri = T.rays_for("a_tiles", 3.0, seed_salt=salt)
        c = cull_check(v, rays[:T.N_RAYS], tri[:T.N_RAYS], kind[:T.N_RAYS], 1)
        p = cull_check(v, rays[:T.N_RAYS], tri[:T.N_RAYS], kind[:T.N_RAYS], 1, build_pad(v))
        tot["hits"] += c["hits"]
        tot["restated"] += c["parent_lost_tmax"]
        tot["restated_t"] += c["parent_lost_t"]
        tot["header"] += c["lost_tmax"]
        tot["header_t"] += c["lost_t"]
        tot["padded"] += p["lost_tmax"] + p["lost_t"] + p["parent_lost_tmax"] + p["parent_lost_t"]
        tot["by_kind"] += np.asarray(c["parent_lost_by_kind"])
    print(tot)
    assert tot["header"] >= 1000, tot
    assert (tot["header"], tot["header_t"]) == (tot["restated"], tot["restated_t"]), tot
    assert tot["by_kind"][T.VERTEX] > 0 and tot["by_kind"][T.EDGE] > 0 and tot["by_kind"][T.INTERIOR] == 0, tot
    assert tot["padded"] == 0, tot
