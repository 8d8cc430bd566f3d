"""CPU restatement of rt_denoise_temporal (csrc/denoise_kernels.h, restir_rt.hip) for tests/test_denoise_temporal_cpu.py and
tests/test_gpu_denoise_temporal.py.

The whole call is restated in plain C++ (whole image, buffer index = row * W + x): the guide from rt_visibility records, the
reprojection into the previous RayGenerator with its four bilinear taps, the integration, the variance (temporal where h >= 4,
k_denoise_var's window elsewhere), the a-trous levels with level 1's output as the next call's colour history, and the output.
Every formula comes from csrc/denoise_math.h; compiled with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit
(rows run on OpenMP threads: every pixel's value is computed by one thread, so the thread count changes nothing).
TemporalRef keeps the history between calls as the context does."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=1.0, normal_power_log2=7, variance_radius=3, alpha_color=0.2,
                alpha_moments=0.2)

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "denoise_math.h"
using namespace rt;

static uint32_t word_of(const float4& gn) { uint32_t w; memcpy(&w, &gn.w, 4); return w; }
static f3 v3(const float4& a) { return F3(a.x, a.y, a.z); }
static f3 albedo(const float* tris, uint32_t word)
{
    const float* t = tris + 15 * (size_t)dn_tri(word);
    return F3(t[9], t[10], t[11]);
}
static float4 f4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

/* k_denoise_guide from the hits */
extern "C" void dnt_guide(int W, int H, const float* tris, const float* vis, const float* eye3, const float* up3, float4* gx, float4* gn)
{
    const size_t n = (size_t)W * H;
    const f3 eye = F3(eye3[0], eye3[1], eye3[2]), up = F3(up3[0], up3[1], up3[2]);
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; ++i)
    {
        int32_t tri;
        memcpy(&tri, vis + 4 * i + 2, 4);
        if (tri < 0)
        {
            const uint32_t w = dn_guide_word(-1, false);
            float wf; memcpy(&wf, &w, 4);
            gx[i] = f4(0.0f, 0.0f, 0.0f, 0.0f);
            gn[i] = f4(0.0f, 0.0f, 0.0f, wf);
            continue;
        }
        const float* t = tris + 15 * (size_t)tri;
        const f3 v0 = F3(t[0], t[1], t[2]), v1 = F3(t[3], t[4], t[5]), v2 = F3(t[6], t[7], t[8]);
        const bool emissive = t[12] > 0.0f || t[13] > 0.0f || t[14] > 0.0f;
        f3 p, nn;
        dn_surface(v0, v1, v2, vis[4 * i], vis[4 * i + 1], eye, p, nn);
        const uint32_t w = dn_guide_word(tri, emissive);
        float wf; memcpy(&wf, &w, 4);
        gx[i] = f4(p.x, p.y, p.z, dn_pixel_size(p, eye, up, H));
        gn[i] = f4(nn.x, nn.y, nn.z, wf);
    }
}

/* dn_window_variance */
static float window_variance(int W, int H, int x, int row, const float4* gx, const float4* gn, const float4* cin, float sigma_x, int npow, int R)
{
    const size_t li = (size_t)x + (size_t)row * W;
    const f3 xp = v3(gx[li]), np = v3(gn[li]);
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
            const float4 cq = cin[qi];
            if (cq.w < 0.0f) continue;
            const float wn = dn_normal_weight(np, v3(gn[qi]), npow);
            const float dxp = dn_plane_distance(np, xp, v3(gx[qi]), sigma_x, 1.0f, gx[li].w);
            dn_moments_add(m, dn_variance_weight(wn, dxp), dn_luminance(cq));
        }
    }
    return dn_moments_variance(m);
}

/* one call. In: the current guide, the accumulation, the previous state (has = 0: none). Out: the HDR image, the new colour
 * history and moments; coords (2 per pixel) = the reprojected (px, pr), NaN where none was computed */
extern "C" void dnt_call(int W, int H, const float* tris, const float4* gx, const float4* gn, const float4* accum, int has,
                         const float* prg, const float4* pgx, const float4* pgn, const float4* hcol, const float4* hmom, float ac,
                         float am, int iterations, float sigma_l, float sigma_x, int npow, int R, float* out, float4* new_hcol,
                         float4* new_mom, float* coords)
{
    const size_t n = (size_t)W * H;
    std::vector<float4> c0(n), c1(n);
    const f3 o = F3(prg[0], prg[1], prg[2]), rr = F3(prg[3], prg[4], prg[5]), uu = F3(prg[6], prg[7], prg[8]);
    /* k_denoise_temporal */
#pragma omp parallel for schedule(static)
    for (int row = 0; row < H; ++row)
        for (int x = 0; x < W; ++x)
        {
            const size_t li = (size_t)x + (size_t)row * W;
            coords[2 * li] = coords[2 * li + 1] = NAN;
            const uint32_t word = word_of(gn[li]);
            const float4 A = accum[li];
            if (dn_kind(word) != DN_KIND_SURFACE || A.w == 0.0f)
            {
                c1[li] = f4(0.0f, 0.0f, 0.0f, -1.0f);
                new_mom[li] = f4(0.0f, 0.0f, 0.0f, 0.0f);
                continue;
            }
            const f3 e = dn_demodulate(A, albedo(tris, word));
            const f3 xp = v3(gx[li]), np = v3(gn[li]);
            DnHistory s = dn_history_init();
            float px, pr;
            if (has && dn_reproject(xp, o, rr, uu, W, H, px, pr))
            {
                coords[2 * li] = px;
                coords[2 * li + 1] = pr;
                int x0, r0;
                float w[4];
                dn_bilinear(px, pr, x0, r0, w);
                for (int k = 0; k < 4; ++k)
                {
                    const int qx = x0 + (k & 1), qr = r0 + (k >> 1);
                    if (qx < 0 || qx >= W || qr < 0 || qr >= H) continue;
                    const size_t qi = (size_t)qx + (size_t)qr * W;
                    if (!dn_temporal_tap_valid(np, xp, gx[li].w, word_of(pgn[qi]), hmom[qi].z, v3(pgn[qi]), v3(pgx[qi]))) continue;
                    dn_history_add(s, w[k], hcol[qi], hmom[qi]);
                }
            }
            float4 c, m;
            dn_temporal_integrate(s, e, ac, am, c, m);
            c1[li] = c;
            new_mom[li] = m;
        }
    /* k_denoise_var_hist: into the colour history itself for 0 iterations */
    float4* vout = iterations == 0 ? new_hcol : c0.data();
#pragma omp parallel for schedule(static)
    for (int row = 0; row < H; ++row)
        for (int x = 0; x < W; ++x)
        {
            const size_t li = (size_t)x + (size_t)row * W;
            const float4 cp = c1[li];
            if (cp.w < 0.0f) { vout[li] = cp; continue; }
            const float4 m = new_mom[li];
            const float var = m.z >= DN_HISTORY_VARIANCE_MIN ? dn_temporal_variance(m) : window_variance(W, H, x, row, gx, gn, c1.data(), sigma_x, npow, R);
            vout[li] = f4(cp.x, cp.y, cp.z, var);
        }
    /* levels: level 1 -> the colour history, level i >= 2 -> c1 / c0 alternately; the last one's input decides pass-through */
    const float4* cin = vout;
    std::vector<unsigned char> part(n);
    for (size_t i = 0; i < n; ++i) part[i] = vout[i].w >= 0.0f;
    for (int it = 0; it < iterations; ++it)
    {
        const int step = 1 << it;
        float4* cout = it == 0 ? new_hcol : ((it & 1) ? c1.data() : c0.data());
#pragma omp parallel for schedule(static)
        for (int row = 0; row < H; ++row)
            for (int x = 0; x < W; ++x)
            {
                const size_t li = (size_t)x + (size_t)row * W;
                const float4 cp = cin[li];
                part[li] = cp.w >= 0.0f;
                if (!part[li]) { cout[li] = cp; continue; }
                auto tap = [&](int dx, int dy, size_t& qi) -> bool {
                    const int qx = x + dx * step, qr = row + dy * step;
                    if (qx < 0 || qx >= W || qr < 0 || qr >= H) return false;
                    qi = (size_t)qx + (size_t)qr * W;
                    return !(cin[qi].w < 0.0f);
                };
                const f3 xp = v3(gx[li]), np = v3(gn[li]);
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
                        const float wn = dn_normal_weight(np, v3(gn[qi]), npow);
                        const float dl = dn_luminance_distance(lp, dn_luminance(cq), sigma_l, gvar);
                        const float dxp = dn_plane_distance(np, xp, v3(gx[qi]), sigma_x, (float)step, gx[li].w);
                        dn_filter_add(f, dn_tap_weight(h, wn, dl, dxp), cq);
                    }
                cout[li] = dn_filter_result(f);
            }
        cin = cout;
    }
    /* output (dn_store<true>) */
    for (size_t i = 0; i < n; ++i)
    {
        float4 v;
        if (part[i]) v = dn_remodulate(cin[i], albedo(tris, word_of(gn[i])));
        else v = accum[i];
        out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
    }
}
"""

_lib = None


def lib():
    """Compile the restatement once per process (g++ -ffp-contract=off, as the host-only units of the project)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="dnt_ref_")
        src, so = os.path.join(d, "dnt_ref.cpp"), os.path.join(d, "dnt_ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, ci, cf = C.c_void_p, C.c_int, C.c_float
        L.dnt_guide.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]
        L.dnt_guide.restype = None
        L.dnt_call.argtypes = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, cf, cf, ci, cf, cf, ci, ci, vp, vp, vp, vp]
        L.dnt_call.restype = None
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def raygen9(rg):
    """origin, right, up of a RayGenerator record (rt_raygen / the oracle's raygen_lookat) as 9 float32"""
    rg = np.asarray(rg)
    if rg.dtype.names:
        return np.concatenate([np.asarray(rg[k], np.float32).reshape(3) for k in ("origin", "right", "up")])
    return np.asarray(rg, np.float32).reshape(9)


class TemporalRef:
    """The context's history and one rt_denoise_temporal call per __call__ (reset() = rt_denoise_temporal_reset)."""

    def __init__(self, W, H, tris, **params):
        self.W, self.H = W, H
        self.tris = np.ascontiguousarray(tris).view(np.uint8)
        self.p = dict(DEFAULTS)
        self.p.update(params)
        self.reset()

    def reset(self):
        self.has = False
        n = self.W * self.H
        self.gx, self.gn, self.hcol, self.hmom = (np.zeros((n, 4), np.float32) for _ in range(4))
        self.rg = np.zeros(9, np.float32)

    def guide(self, vis, eye, rg):
        n = self.W * self.H
        v = np.ascontiguousarray(vis).view(np.uint8)
        assert v.nbytes == 16 * n
        gx, gn = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        e = np.asarray(eye, np.float32).reshape(3)
        lib().dnt_guide(self.W, self.H, _ptr(self.tris), _ptr(v), _ptr(e), _ptr(raygen9(rg)[6:9].copy()), _ptr(gx), _ptr(gn))
        return gx, gn

    def __call__(self, vis, eye, rg, accum, **params):
        """One frame: `vis` = the guide's hits (rt_visibility records of the current camera), eye / rg = the current camera,
        accum = the accumulation buffer. Returns the HDR image (W * H, 4) and the moments {mu1, mu2, h, 0} (RT_BUF_DENOISE_HISTORY);
        self.coords holds the reprojected (px, pr) per pixel (NaN where none)."""
        p = dict(self.p)
        p.update(params)
        n = self.W * self.H
        gx, gn = self.guide(vis, eye, rg)
        a = np.ascontiguousarray(accum, dtype=np.float32).reshape(-1, 4)
        assert len(a) == n
        out, hcol, mom = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        coords = np.zeros((n, 2), np.float32)
        lib().dnt_call(self.W, self.H, _ptr(self.tris), _ptr(gx), _ptr(gn), _ptr(a), int(self.has), _ptr(self.rg), _ptr(self.gx),
                       _ptr(self.gn), _ptr(self.hcol), _ptr(self.hmom), float(p["alpha_color"]), float(p["alpha_moments"]),
                       int(p["iterations"]), float(p["sigma_luminance"]), float(p["sigma_plane"]), int(p["normal_power_log2"]),
                       int(p["variance_radius"]), _ptr(out), _ptr(hcol), _ptr(mom), _ptr(coords))
        self.gx, self.gn, self.hcol, self.hmom, self.rg = gx, gn, hcol, mom, raygen9(rg).copy()
        self.has = True
        self.coords = coords
        self.words = gn[:, 3].view(np.uint32).copy()
        return out, mom
