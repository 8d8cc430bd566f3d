"""CPU restatement of rt_denoise (csrc/denoise_kernels.h) for tests/test_denoise_cpu.py and tests/test_gpu_denoise.py.

The loops are restated here in plain C++ (whole image, buffer index = row * W + x, taps dy outer and dx inner); every formula comes
from csrc/denoise_math.h. Compiled with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit. The guide is built
from rt_visibility records (the oracle's raycast, or the GPU's RT_BUF_DENOISE_GUIDE) and the scene's triangles."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=1.0, normal_power_log2=7, variance_radius=3)

PROGRAM = r"""
#include <cstdint>
#include <cstring>
#include <vector>
#include "denoise_math.h"
using namespace rt;

struct Px { float4 gx, gn; };

static f3 albedo(const float* tris, uint32_t word)
{
    const float* t = tris + 15 * (size_t)dn_tri(word);
    return F3(t[9], t[10], t[11]);
}

extern "C" void dn_ref(int W, int H, const float* tris, const float* vis, const float* eye3, const float* up3, const float* accum,
                       int iterations, float sigma_l, float sigma_x, int npow, int R, float* out, uint32_t* words)
{
    const size_t n = (size_t)W * H;
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]), up = F3(up3[0], up3[1], up3[2]);
    std::vector<Px> g(n);
    std::vector<float4> c0(n), c1(n);
    /* guide */
    for (size_t i = 0; i < n; ++i)
    {
        int32_t tri;
        memcpy(&tri, vis + 4 * i + 2, 4);
        if (tri < 0)
        {
            g[i].gx = float4{0.0f, 0.0f, 0.0f, 0.0f};
            uint32_t w = dn_guide_word(-1, false);
            float wf; memcpy(&wf, &w, 4);
            g[i].gn = float4{0.0f, 0.0f, 0.0f, wf};
            continue;
        }
        const float* t = tris + 15 * (size_t)tri;
        const f3 v0 = F3(t[0], t[1], t[2]), v1 = F3(t[3], t[4], t[5]), v2 = F3(t[6], t[7], t[8]);
        const bool emissive = t[12] > 0.0f || t[13] > 0.0f || t[14] > 0.0f;
        f3 p, nn;
        dn_surface(v0, v1, v2, vis[4 * i], vis[4 * i + 1], eye, p, nn);
        g[i].gx = float4{p.x, p.y, p.z, dn_pixel_size(p, eye, up, H)};
        uint32_t w = dn_guide_word(tri, emissive);
        float wf; memcpy(&wf, &w, 4);
        g[i].gn = float4{nn.x, nn.y, nn.z, wf};
    }
    auto word_of = [&](size_t i) { uint32_t w; memcpy(&w, &g[i].gn.w, 4); return w; };
    if (words) for (size_t i = 0; i < n; ++i) words[i] = word_of(i);
    /* demodulation */
    for (size_t i = 0; i < n; ++i)
    {
        const float4 A = float4{accum[4 * i], accum[4 * i + 1], accum[4 * i + 2], accum[4 * i + 3]};
        const uint32_t w = word_of(i);
        if (dn_kind(w) != DN_KIND_SURFACE || A.w == 0.0f) { c1[i] = float4{0.0f, 0.0f, 0.0f, -1.0f}; continue; }
        const f3 e = dn_demodulate(A, albedo(tris, w));
        c1[i] = float4{e.x, e.y, e.z, 0.0f};
    }
    /* variance */
    for (int row = 0; row < H; ++row)
        for (int x = 0; x < W; ++x)
        {
            const size_t li = (size_t)x + (size_t)row * W;
            const float4 cp = c1[li];
            if (cp.w < 0.0f) { c0[li] = cp; continue; }
            const f3 xp = F3(g[li].gx.x, g[li].gx.y, g[li].gx.z), np = F3(g[li].gn.x, g[li].gn.y, g[li].gn.z);
            DnMoments m = dn_moments_init();
            for (int dy = -R; dy <= R; ++dy)
            {
                const int qr = row + dy;
                if (qr < 0 || qr >= H) continue;
                for (int dx = -R; dx <= R; ++dx)
                {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= W) continue;
                    const size_t qi = (size_t)qx + (size_t)qr * W;
                    const float4 cq = c1[qi];
                    if (cq.w < 0.0f) continue;
                    const float wn = dn_normal_weight(np, F3(g[qi].gn.x, g[qi].gn.y, g[qi].gn.z), npow);
                    const float dxp = dn_plane_distance(np, xp, F3(g[qi].gx.x, g[qi].gx.y, g[qi].gx.z), sigma_x, 1.0f, g[li].gx.w);
                    dn_moments_add(m, dn_variance_weight(wn, dxp), dn_luminance(cq));
                }
            }
            c0[li] = float4{cp.x, cp.y, cp.z, dn_moments_variance(m)};
        }
    /* levels */
    std::vector<float4>* cur = &c0;
    std::vector<float4>* nxt = &c1;
    for (int it = 0; it < iterations; ++it)
    {
        const int step = 1 << it;
        const std::vector<float4>& cin = *cur;
        std::vector<float4>& cout = *nxt;
        for (int row = 0; row < H; ++row)
            for (int x = 0; x < W; ++x)
            {
                const size_t li = (size_t)x + (size_t)row * W;
                const float4 cp = cin[li];
                if (cp.w < 0.0f) { cout[li] = cp; continue; }
                auto tap = [&](int dx, int dy, size_t& qi) -> bool {
                    const int qx = x + dx * step, qr = row + dy * step;
                    if (qx < 0 || qx >= W || qr < 0 || qr >= H) return false;
                    qi = (size_t)qx + (size_t)qr * W;
                    return !(cin[qi].w < 0.0f);
                };
                const f3 xp = F3(g[li].gx.x, g[li].gx.y, g[li].gx.z), np = F3(g[li].gn.x, g[li].gn.y, g[li].gn.z);
                DnPrefilter pf = dn_prefilter_init();
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                    {
                        size_t qi;
                        if (tap(dx, dy, qi)) dn_prefilter_add(pf, dn_k1(dx) * dn_k1(dy), cin[qi].w);
                    }
                const float gvar = dn_prefilter_result(pf);
                const float lp = dn_luminance(cp);
                DnFilter f = dn_filter_init();
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx)
                    {
                        size_t qi;
                        if (!tap(dx, dy, qi)) continue;
                        const float4 cq = cin[qi];
                        const float h = dn_h1(dx) * dn_h1(dy);
                        const float wn = dn_normal_weight(np, F3(g[qi].gn.x, g[qi].gn.y, g[qi].gn.z), npow);
                        const float dl = dn_luminance_distance(lp, dn_luminance(cq), sigma_l, gvar);
                        const float dxp = dn_plane_distance(np, xp, F3(g[qi].gx.x, g[qi].gx.y, g[qi].gx.z), sigma_x, (float)step, g[li].gx.w);
                        dn_filter_add(f, dn_tap_weight(h, wn, dl, dxp), cq);
                    }
                cout[li] = dn_filter_result(f);
            }
        std::swap(cur, nxt);
    }
    /* output */
    for (size_t i = 0; i < n; ++i)
    {
        const float4 e = (*cur)[i];
        float4 v;
        if (e.w >= 0.0f) v = dn_remodulate(e, albedo(tris, word_of(i)));
        else v = float4{accum[4 * i], accum[4 * i + 1], accum[4 * i + 2], accum[4 * i + 3]};
        out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
    }
}
"""

_lib = None


def lib():
    """Compile the restatement once per process (g++ -ffp-contract=off, as the host-only units of the project)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="dn_ref_")
        src, so = os.path.join(d, "dn_ref.cpp"), os.path.join(d, "dn_ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.dn_ref.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, vp, vp]
        L.dn_ref.restype = None
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def denoise(W, H, tris, vis, eye, rg_up, accum, words=False, **params):
    """HDR result (W * H, 4) float32 of rt_denoise for the accumulation buffer `accum` and the guide hits `vis` (rt_visibility
    records, storage order). eye = the camera's eye, rg_up = the RayGenerator's up vector. words=True also returns the guide words."""
    p = dict(DEFAULTS)
    p.update(params)
    t = np.ascontiguousarray(tris).view(np.uint8)
    v = np.ascontiguousarray(vis).view(np.uint8)
    a = np.ascontiguousarray(accum, dtype=np.float32).reshape(-1, 4)
    assert len(a) == W * H and v.nbytes == 16 * W * H
    e = np.asarray(eye, dtype=np.float32).reshape(3)
    u = np.asarray(rg_up, dtype=np.float32).reshape(3)
    out = np.zeros((W * H, 4), dtype=np.float32)
    w = np.zeros(W * H, dtype=np.uint32)
    lib().dn_ref(W, H, _ptr(t), _ptr(v), _ptr(e), _ptr(u), _ptr(a), int(p["iterations"]), float(p["sigma_luminance"]),
                 float(p["sigma_plane"]), int(p["normal_power_log2"]), int(p["variance_radius"]), _ptr(out), _ptr(w))
    return (out, w) if words else out
