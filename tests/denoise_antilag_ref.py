"""CPU restatement of rt_denoise_temporal under rt_denoise_temporal_antilag (csrc/denoise_antilag.h, csrc/denoise_kernels.h,
restir_rt.hip) for tests/test_denoise_antilag_cpu.py and tests/test_gpu_denoise_antilag.py.

The C++ is tests/denoise_motion_ref.py's program (itself tests/denoise_temporal_ref.py's with the followed lookup) with the places an
adapted call differs, so it covers followed calls as well: in an adapted call (the toggle on and a history) the first loop keeps what
k_denoise_antilag_gather keeps ({e, l_h}, the history's quotients, the previous moments) and a second loop restates
k_denoise_antilag: the window in the order dy outer, dx inner, lambda', the blend. Every formula comes from csrc/denoise_antilag.h;
compiled with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit.

AntilagRef is MotionRef with the toggle and its parameters; after a call self.grad (n, 4) float32 holds {mc, mh, members, lambda}
of the pixels that formed a window (NaN elsewhere) and the moments' fourth component lambda'."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import denoise_motion_ref as dm
import denoise_temporal_ref as dtr

DEFAULTS = dict(radius=4, gradient_lo=0.2, gradient_hi=0.8, floor=0.05)

_SIG_OLD = "const float* tris_prev, const float* vis, int* diag)"
_SIG_NEW = ("const float* tris_prev, const float* vis, int* diag,\n                         int antilag, int al_radius, float al_lo, float al_hi, "
            "float al_floor, float* grad)")
_SKIP_OLD = "                c1[li] = f4(0.0f, 0.0f, 0.0f, -1.0f);\n                new_mom[li] = f4(0.0f, 0.0f, 0.0f, 0.0f);\n                continue;"
_SKIP_NEW = ("                c0[li] = f4(0.0f, 0.0f, 0.0f, -1.0f);\n"
             "                grad[4 * li] = grad[4 * li + 1] = grad[4 * li + 2] = grad[4 * li + 3] = NAN;\n" + _SKIP_OLD)
_INT_OLD = """            float4 c, m;
            dn_temporal_integrate(s, e, ac, am, c, m);
            c1[li] = c;
            new_mom[li] = m;
        }
"""
_INT_NEW = r"""            grad[4 * li] = grad[4 * li + 1] = grad[4 * li + 2] = grad[4 * li + 3] = NAN;
            if (antilag && has)
            {
                /* k_denoise_antilag_gather: {e, l_h} -> c0, {c_prev, 0} -> c1, the previous moments -> new_mom */
                float4 c = f4(0.0f, 0.0f, 0.0f, 0.0f), m = f4(0.0f, 0.0f, 0.0f, 0.0f);
                float lh = -1.0f;
                if (s.sw >= DN_TEMPORAL_WEIGHT_MIN)
                {
                    c = f4(s.r / s.sw, s.g / s.sw, s.b / s.sw, 0.0f);
                    m = f4(s.m1 / s.sw, s.m2 / s.sw, s.h, 0.0f);
                    lh = dn_luminance(c);
                }
                c0[li] = f4(e.x, e.y, e.z, lh);
                c1[li] = c;
                new_mom[li] = m;
                continue;
            }
            float4 c, m;
            dn_temporal_integrate(s, e, ac, am, c, m);
            c1[li] = c;
            new_mom[li] = m;
        }
    /* k_denoise_antilag */
    if (antilag && has)
    {
        const int R = al_radius;
#pragma omp parallel for schedule(static)
        for (int row = 0; row < H; ++row)
            for (int x = 0; x < W; ++x)
            {
                const size_t li = (size_t)x + (size_t)row * W;
                if (c1[li].w < 0.0f) continue;
                const float4 ep = c0[li];
                const f3 e = F3(ep.x, ep.y, ep.z);
                float4 c, m;
                if (!dn_antilag_has_history(ep.w)) dn_antilag_first(e, c, m);
                else
                {
                    const f3 np = v3(gn[li]);
                    DnGradient g = dn_gradient_init();
                    for (int dy = -R; dy <= R; ++dy)
                        for (int dx = -R; dx <= R; ++dx)
                        {
                            const int qx = x + dx, qr = row + dy;
                            if (qx < 0 || qx >= W || qr < 0 || qr >= H) continue;
                            const size_t qi = (size_t)qx + (size_t)qr * W;
                            if (dn_antilag_member(np, v3(gn[qi]), c0[qi].w)) dn_gradient_add(g, dn_luminance(c0[qi]), c0[qi].w);
                        }
                    const float lambda = dn_gradient_lambda(g, al_floor);
                    grad[4 * li] = g.mc; grad[4 * li + 1] = g.mh; grad[4 * li + 2] = (float)g.n; grad[4 * li + 3] = lambda;
                    dn_antilag_integrate(c1[li], new_mom[li], e, ac, am, dn_antilag_response(lambda, al_lo, al_hi), c, m);
                }
                c1[li] = c;
                new_mom[li] = m;
            }
    }
"""


def _program():
    p = dm._program()
    for old, new in ((_SIG_OLD, _SIG_NEW), (_SKIP_OLD, _SKIP_NEW), (_INT_OLD, _INT_NEW)):
        assert p.count(old) == 1, "tests/denoise_motion_ref.py or tests/denoise_temporal_ref.py changed: " + old
        p = p.replace(old, new)
    p = p.replace('#include "denoise_motion.h"', '#include "denoise_motion.h"\n#include "denoise_antilag.h"')
    for name in ("call", "guide", "followed"):
        assert p.count('extern "C" void dnm_%s(' % name) + p.count('extern "C" int dnm_%s(' % name) == 1
        p = p.replace("dnm_%s(" % name, "dna_%s(" % name)
    return p


_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="dna_ref_")
        src, so = os.path.join(d, "dna_ref.cpp"), os.path.join(d, "dna_ref.so")
        with open(src, "w") as f:
            f.write(_program())
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-I", dtr.CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, ci, cf, u32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_uint64
        L.dna_guide.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]
        L.dna_guide.restype = None
        L.dna_call.argtypes = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, cf, cf, ci, cf, cf, ci, ci, vp, vp, vp, vp, ci, vp, u32, u32, vp, vp, vp,
                               ci, ci, cf, cf, cf, vp]
        L.dna_call.restype = None
        L.dna_followed.argtypes = [ci, ci, ci, u64, u64, u64]
        L.dna_followed.restype = ci
        _lib = L
    return _lib


_ptr = dtr._ptr


class AntilagRef(dm.MotionRef):
    """MotionRef (`on` = rt_denoise_temporal_motion) with rt_denoise_temporal_antilag: antilag = the toggle, al = its parameters"""

    def __init__(self, W, H, tris, on=False, motion=False, antilag=False, al=None, **params):
        super().__init__(W, H, tris, on=on, motion=motion, **params)
        self.antilag, self.al = bool(antilag), dict(DEFAULTS)
        self.al.update(al or {})
        self.adapted = False

    def toggle_antilag(self, on, **al):
        """rt_denoise_temporal_antilag: host state only"""
        self.antilag = bool(on)
        self.al.update(al)

    def __call__(self, vis, eye, rg, accum, **params):
        """As MotionRef.__call__; afterwards also self.adapted and self.grad"""
        p = dict(self.p)
        p.update(params)
        n = self.W * self.H
        L = lib()
        gx, gn = self.guide(vis, eye, rg)
        a = np.ascontiguousarray(accum, dtype=np.float32).reshape(-1, 4)
        assert len(a) == n
        v = np.ascontiguousarray(vis).view(np.uint8)
        out, hcol, mom = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        scratch = np.full(8 * n, np.nan, np.float32)
        diag = np.zeros((n, 4), np.int32)
        grad = np.full((n, 4), np.nan, np.float32)
        followed = bool(L.dna_followed(int(self.on), int(self.has), int(self.tv_prev is not None), self.dt_gen, self.tvp_gen, self.geo_gen))
        prev = self.tv_prev if followed else self.tris
        adapted = self.antilag and self.has
        L.dna_call(self.W, self.H, _ptr(self.tris), _ptr(gx), _ptr(gn), _ptr(a), int(self.has), _ptr(self.rg), _ptr(self.gx),
                   _ptr(self.gn), _ptr(self.hcol), _ptr(self.hmom), float(p["alpha_color"]), float(p["alpha_moments"]),
                   int(p["iterations"]), float(p["sigma_luminance"]), float(p["sigma_plane"]), int(p["normal_power_log2"]),
                   int(p["variance_radius"]), _ptr(out), _ptr(hcol), _ptr(mom), _ptr(scratch), int(followed), _ptr(self.dt_eye),
                   self.lo, self.hi, _ptr(prev), _ptr(v), _ptr(diag), int(self.antilag), int(self.al["radius"]),
                   float(self.al["gradient_lo"]), float(self.al["gradient_hi"]), float(self.al["floor"]), _ptr(grad))
        self.gx, self.gn, self.hcol, self.hmom, self.rg = gx, gn, hcol, mom, dtr.raygen9(rg).copy()
        self.has = True
        self.dt_gen, self.dt_eye = self.geo_gen, np.asarray(eye, np.float32).reshape(3).copy()
        if self.on:
            self.dt_dirty = True
        self.followed, self.adapted = followed, bool(adapted)
        self.coords, self.lookup, self.diag = scratch[:2 * n].reshape(n, 2).copy(), scratch[2 * n:].reshape(n, 6).copy(), diag
        self.grad = grad
        self.words = gn[:, 3].view(np.uint32).copy()
        return out, mom
