"""CPU restatement of rt_temporal_light_motion (csrc/light_follow.h) for tests/test_light_follow_cpu.py and
tests/test_gpu_light_follow.py, after the pattern of tests/temporal_motion_ref.py.

One re-basing of a reservoir buffer in plain C++ on the reference's 76-byte Reservoir records. Every formula comes from
csrc/light_follow.h and csrc/rt_device.h, the headers the kernel is compiled from; built with `g++ -ffp-contract=off`, so the result
equals the GPU's bit for bit. It locates by a brute-force loop over every triangle of the span, where the kernel queries the old tree
or loops over the span's light list.

A 76-byte record has neither the shaded bit nor a stored luminance: a record is examined iff M > 0 (the kernels leave Reservoir{} in
every pixel that is not shaded), and luminance(radiance) is what a reader of the record computes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "rt_device.h"
#include "light_follow.h"
using namespace rt;

struct Tri { float v[9], color[3], emissive[3]; };
struct Reservoir
{
    float origin_position[3], origin_normal[3], hit_position[3], hit_normal[3], radiance[3];
    uint8_t visibility, pad[3];
    float w_sum, ucw;
    int32_t M;
};
static_assert(sizeof(Tri) == 60 && sizeof(Reservoir) == 76, "the reference's PODs");
static f3 v3(const float* a) { return F3(a[0], a[1], a[2]); }

/* located[i]: the triangle record i was located on, -1 if none (or not examined); uv[2 i], uv[2 i + 1]: its barycentrics there;
 * counts: examined, located, moved, emptied */
extern "C" void lf_rebase(int n, Reservoir* res, const Tri* tris_old, const Tri* tris_new_span, uint32_t first, uint32_t count, int jacobian,
                          int32_t* located, float* uv, uint64_t* counts)
{
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int i = 0; i < n; ++i)
    {
        located[i] = -1; uv[2 * i] = uv[2 * i + 1] = 0.0f;
        Reservoir& r = res[i];
        if (r.M <= 0) continue;
        ++counts[0];
        LfMatch best;
        memset(&best, 0, sizeof(best));
        int best_t = -1;
        for (uint32_t t = first; t < first + count; ++t)
        {
            const Tri& o = tris_old[t];
            const LfMatch m = lf_locate_test(v3(r.hit_position), v3(r.hit_normal), v3(r.radiance), v3(o.v), v3(o.v + 3), v3(o.v + 6), v3(o.emissive));
            if (lf_better(m, (int)t, best, best_t)) { best = m; best_t = (int)t; }
        }
        if (best_t < 0) continue;
        ++counts[1];
        located[i] = best_t; uv[2 * i] = best.u; uv[2 * i + 1] = best.v;
        LfSample s;
        s.hit_p = v3(r.hit_position); s.hit_n = v3(r.hit_normal); s.rad = v3(r.radiance); s.ucw = r.ucw; s.lum = 0.0f;
        const LfOutcome out = lf_apply(s, best, tris_old[best_t].v, tris_new_span[best_t - first].v, jacobian != 0);
        if (out == LF_MOVED)
        {
            ++counts[2];
            r.hit_position[0] = s.hit_p.x; r.hit_position[1] = s.hit_p.y; r.hit_position[2] = s.hit_p.z;
            r.hit_normal[0] = s.hit_n.x; r.hit_normal[1] = s.hit_n.y; r.hit_normal[2] = s.hit_n.z;
            r.radiance[0] = s.rad.x; r.radiance[1] = s.rad.y; r.radiance[2] = s.rad.z;
            r.ucw = s.ucw;
        }
        else if (out == LF_EMPTIED)
        {
            ++counts[3];
            memset(&r, 0, sizeof(r));
        }
    }
}
extern "C" float lf_tau_p() { return LF_TAU_P; }
extern "C" float lf_tau_b() { return LF_TAU_B; }
/* the binary32 plane distance over the triangle's largest |coordinate|, and the barycentrics, of point p on triangle t, as
 * lf_locate_test computes them (no acceptance): for the measurement of the tolerances */
extern "C" void lf_measure(int n, const float* p, const Tri* t, float* out3)
{
    for (int i = 0; i < n; ++i)
    {
        const f3 v0 = v3(t[i].v), v1 = v3(t[i].v + 3), v2 = v3(t[i].v + 6), hp = v3(p + 3 * i);
        const f3 e1 = v1 - v0, e2 = v2 - v0, c = cross(e1, e2);
        const f3 nn = c / length(c), d = hp - v0;
        out3[3 * i] = fabsf(dot(nn, d)) / lf_max_abs(v0, v1, v2);
        const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), dp1 = dot(d, e1), dp2 = dot(d, e2);
        const float det = d11 * d22 - d12 * d12;
        out3[3 * i + 1] = (d22 * dp1 - d12 * dp2) / det;
        out3[3 * i + 2] = (d11 * dp2 - d12 * dp1) / det;
    }
}
"""

_lib = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lib():
    """the restatement, compiled once per process into a temporary directory"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="light_follow_ref_")
        src, so = os.path.join(d, "ref.cpp"), os.path.join(d, "ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
        L = C.CDLL(so)
        vp, ci, cu = C.c_void_p, C.c_int, C.c_uint32
        L.lf_rebase.argtypes = [ci, vp, vp, vp, cu, cu, ci, vp, vp, vp]
        L.lf_rebase.restype = None
        L.lf_measure.argtypes = [ci, vp, vp, vp]
        L.lf_measure.restype = None
        L.lf_tau_p.restype = C.c_float
        L.lf_tau_b.restype = C.c_float
        _lib = L
    return _lib


def tau():
    """(LF_TAU_P, LF_TAU_B) of csrc/light_follow.h"""
    return float(lib().lf_tau_p()), float(lib().lf_tau_b())


def rebase(res, tris_old, tris_new, first, count, jacobian=True):
    """What rt_scene_update(tris_new[first:first + count], first, count) does to a qualifying reservoir buffer while the toggle is on.
    res: the oracle's RESERVOIR array (not modified); tris_old / tris_new: whole TRIANGLE arrays before and after the update (same count
    and order; only the span may differ). Returns (res', located (n,) int32, uv (n, 2) float32, counts dict). jacobian=False plants the
    error of the Jacobian test: the area factor left out."""
    tris_old, tris_new = np.ascontiguousarray(tris_old), np.ascontiguousarray(tris_new)
    assert tris_old.dtype.itemsize == 60 and tris_new.dtype.itemsize == 60 and len(tris_old) == len(tris_new)
    assert res.dtype.itemsize == 76 and 0 <= first and first + count <= len(tris_old)
    out = np.ascontiguousarray(res).copy()
    span = np.ascontiguousarray(tris_new[first:first + count])
    located = np.zeros(len(out), np.int32)
    uv = np.zeros((len(out), 2), np.float32)
    counts = np.zeros(4, np.uint64)
    lib().lf_rebase(len(out), _p(out), _p(tris_old), _p(span), int(first), int(count), int(bool(jacobian)), _p(located), _p(uv), _p(counts))
    return out, located, uv, dict(zip(("examined", "located", "moved", "emptied"), (int(x) for x in counts)))


def measure(points, tris):
    """(n, 3) float32: the binary32 plane term and barycentrics of points[i] on tris[i], as lf_locate_test computes them"""
    points, tris = np.ascontiguousarray(points, dtype=np.float32), np.ascontiguousarray(tris)
    out = np.zeros((len(points), 3), np.float32)
    lib().lf_measure(len(points), _p(points), _p(tris), _p(out))
    return out
