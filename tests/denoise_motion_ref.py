"""CPU restatement of rt_denoise_temporal under rt_denoise_temporal_motion (csrc/denoise_motion.h, csrc/denoise_kernels.h,
restir_rt.hip) for tests/test_denoise_motion_cpu.py and tests/test_gpu_denoise_motion.py.

The C++ is tests/denoise_temporal_ref.py's program with the one place a followed call differs: before dn_reproject a participating
pixel whose triangle lies in the moved range takes its lookup point and normal from dn_motion_lookup (tm_previous_surface on the
triangle's previous vertices, the (u, v) of this call's guide hit, the previous call's eye); reprojection and the four taps then run
on them. Compiled from the project's headers with `g++ -ffp-contract=off`, so the result equals the GPU's bit for bit.

MotionRef keeps the history between calls as TemporalRef does, and also what the context keeps by the host rules: the geometry
generation, the generation and the vertices the kept previous triangles describe, the moved range, the two dirty flags and both
toggles (rt_temporal_motion shares the kept vertices; frame() stands for a frame that tags a reservoir buffer)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import denoise_temporal_ref as dtr

_SIG_OLD = "float* out, float4* new_hcol,\n                         float4* new_mom, float* coords)"
_SIG_NEW = ("float* out, float4* new_hcol,\n                         float4* new_mom, float* coords, int followed, const float* eye_prev3, "
            "uint32_t lo, uint32_t hi,\n                         const float* tris_prev, const float* vis, int* diag)")
_PIX_OLD = "            const f3 xp = v3(gx[li]), np = v3(gn[li]);\n            DnHistory s = dn_history_init();"
_PIX_NEW = r"""            f3 xp = v3(gx[li]), np = v3(gn[li]); /* the lookup point and normal */
            diag[4 * li] = 0; diag[4 * li + 1] = 0; diag[4 * li + 2] = -1; diag[4 * li + 3] = -1;
            if (followed)
            {
                const int prim = dn_tri(word);
                if (tm_in_range(prim, lo, hi))
                {
                    const float* t = tris_prev + 15 * (size_t)prim;
                    dn_motion_lookup(F3(t[0], t[1], t[2]), F3(t[3], t[4], t[5]), F3(t[6], t[7], t[8]), vis[4 * li], vis[4 * li + 1],
                                     F3(eye_prev3[0], eye_prev3[1], eye_prev3[2]), xp, np);
                    diag[4 * li] = 1;
                    lookup[6 * li] = xp.x; lookup[6 * li + 1] = xp.y; lookup[6 * li + 2] = xp.z;
                    lookup[6 * li + 3] = np.x; lookup[6 * li + 4] = np.y; lookup[6 * li + 5] = np.z;
                }
            }
            float wbest = 0.0f;
            DnHistory s = dn_history_init();"""
_TAP_OLD = "                    dn_history_add(s, w[k], hcol[qi], hmom[qi]);"
_TAP_NEW = r"""                    dn_history_add(s, w[k], hcol[qi], hmom[qi]);
                    diag[4 * li + 1] += 1;
                    if (w[k] > wbest) { wbest = w[k]; diag[4 * li + 2] = qx; diag[4 * li + 3] = qr; }"""


def _program():
    p = dtr.PROGRAM
    for old, new in ((_SIG_OLD, _SIG_NEW + "\n{\n    float* lookup = coords + 2 * (size_t)W * H;\n    dnm_body"), (_PIX_OLD, _PIX_NEW), (_TAP_OLD, _TAP_NEW)):
        assert p.count(old) == 1, "tests/denoise_temporal_ref.py changed: " + old
        p = p.replace(old, new)
    # the opening brace of the function now follows the inserted line: `dnm_body` marks it
    assert p.count("dnm_body\n{\n") == 1
    p = p.replace("dnm_body\n{\n", "")
    p = p.replace('#include "denoise_math.h"', '#include "denoise_math.h"\n#include "denoise_motion.h"')
    p = p.replace('extern "C" void dnt_call(', 'extern "C" void dnm_call(').replace('extern "C" void dnt_guide(', 'extern "C" void dnm_guide(')
    return p + r"""
extern "C" int dnm_followed(int toggle, int has, int have_prev, uint64_t hist_gen, uint64_t prev_gen, uint64_t cur_gen)
{
    return dn_motion_followed(toggle != 0, has != 0, have_prev != 0, hist_gen, prev_gen, cur_gen) ? 1 : 0;
}
"""


_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="dnm_ref_")
        src, so = os.path.join(d, "dnm_ref.cpp"), os.path.join(d, "dnm_ref.so")
        with open(src, "w") as f:
            f.write(_program())
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-I", dtr.CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, ci, cf, u32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_uint64
        L.dnm_guide.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp]
        L.dnm_guide.restype = None
        L.dnm_call.argtypes = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, cf, cf, ci, cf, cf, ci, ci, vp, vp, vp, vp, ci, vp, u32, u32, vp, vp, vp]
        L.dnm_call.restype = None
        L.dnm_followed.argtypes = [ci, ci, ci, u64, u64, u64]
        L.dnm_followed.restype = ci
        _lib = L
    return _lib


_ptr = dtr._ptr


def _bytes(tris):
    return np.ascontiguousarray(tris).view(np.uint8).copy()


class MotionRef:
    """The context's denoiser history and scene bookkeeping; one rt_denoise_temporal call per __call__."""

    def __init__(self, W, H, tris, on=False, motion=False, **params):
        self.W, self.H = W, H
        self.p = dict(dtr.DEFAULTS)
        self.p.update(params)
        self.on, self.motion = False, False
        self.tv_prev = None
        self.followed = False
        self.set_scene(tris)
        self.toggle(on)
        self.toggle_motion(motion)

    # ---- host rules (restir_rt.hip) ----
    def set_scene(self, tris):
        """rt_scene_set: generations count from 0, the history is empty, the kept vertices are made anew while either toggle is on"""
        self.tris = _bytes(tris)
        self.n_tris = len(tris)
        self.geo_gen, self.res_dirty, self.dt_dirty = 0, False, False
        self.reset()
        self._rebase_all()

    def _rebase_all(self):
        self.tvp_gen, self.lo, self.hi = self.geo_gen, 0, 0
        self.tv_prev = self.tris.copy() if (self.on or self.motion) else None

    def toggle(self, on):
        """rt_denoise_temporal_motion"""
        was, self.on = self.on, bool(on)
        if self.on == was:
            return
        self.dt_dirty = False
        if not self.motion:
            self._rebase_all()

    def toggle_motion(self, on):
        """rt_temporal_motion, as far as the kept vertices go"""
        was, self.motion = self.motion, bool(on)
        if self.motion != was and not self.on:
            self._rebase_all()

    def frame(self):
        """a frame (or any call that tags a reservoir buffer)"""
        self.res_dirty = True

    def update(self, span, first):
        """rt_scene_update(span, first, len(span))"""
        count = len(span)
        rec = self.tris.reshape(self.n_tris, 60)
        if self.tv_prev is not None:
            if (self.motion and self.res_dirty) or (self.on and self.dt_dirty):
                if self.hi > self.lo:
                    self.tv_prev.reshape(self.n_tris, 60)[self.lo:self.hi] = rec[self.lo:self.hi]
                self.tvp_gen, self.lo, self.hi = self.geo_gen, first, first + count
            elif self.hi > self.lo:
                self.lo, self.hi = min(self.lo, first), max(self.hi, first + count)
            else:
                self.lo, self.hi = first, first + count
        self.geo_gen += 1
        self.res_dirty = self.dt_dirty = False
        rec[first:first + count] = _bytes(span).reshape(count, 60)

    def range(self):
        return dict(lo=self.lo, hi=self.hi, generation=self.tvp_gen)

    def reset(self):
        """rt_denoise_temporal_reset"""
        self.has = False
        n = self.W * self.H
        self.gx, self.gn, self.hcol, self.hmom = (np.zeros((n, 4), np.float32) for _ in range(4))
        self.rg = np.zeros(9, np.float32)
        self.dt_gen, self.dt_eye = 0, np.zeros(3, np.float32)

    # ---- the call ----
    def guide(self, vis, eye, rg):
        n = self.W * self.H
        v = np.ascontiguousarray(vis).view(np.uint8)
        assert v.nbytes == 16 * n
        gx, gn = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        e = np.asarray(eye, np.float32).reshape(3)
        lib().dnm_guide(self.W, self.H, _ptr(self.tris), _ptr(v), _ptr(e), _ptr(dtr.raygen9(rg)[6:9].copy()), _ptr(gx), _ptr(gn))
        return gx, gn

    def __call__(self, vis, eye, rg, accum, **params):
        """As TemporalRef.__call__. Afterwards: self.followed (a followed call), self.diag (n, 4) int32 = {on the moved range, valid
        taps, x and row of the valid tap with the largest weight or -1}, self.coords (px, pr) of the lookup point, self.lookup (n, 6) =
        (x_l, n_l) of the pixels on the range (NaN elsewhere)."""
        p = dict(self.p)
        p.update(params)
        n = self.W * self.H
        L = lib()
        gx, gn = self.guide(vis, eye, rg)
        a = np.ascontiguousarray(accum, dtype=np.float32).reshape(-1, 4)
        assert len(a) == n
        v = np.ascontiguousarray(vis).view(np.uint8)
        out, hcol, mom = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        scratch = np.full(8 * n, np.nan, np.float32)  # coords (2 n) then lookup (6 n)
        diag = np.zeros((n, 4), np.int32)
        followed = bool(L.dnm_followed(int(self.on), int(self.has), int(self.tv_prev is not None), self.dt_gen, self.tvp_gen, self.geo_gen))
        prev = self.tv_prev if followed else self.tris
        L.dnm_call(self.W, self.H, _ptr(self.tris), _ptr(gx), _ptr(gn), _ptr(a), int(self.has), _ptr(self.rg), _ptr(self.gx),
                   _ptr(self.gn), _ptr(self.hcol), _ptr(self.hmom), float(p["alpha_color"]), float(p["alpha_moments"]),
                   int(p["iterations"]), float(p["sigma_luminance"]), float(p["sigma_plane"]), int(p["normal_power_log2"]),
                   int(p["variance_radius"]), _ptr(out), _ptr(hcol), _ptr(mom), _ptr(scratch), int(followed), _ptr(self.dt_eye),
                   self.lo, self.hi, _ptr(prev), _ptr(v), _ptr(diag))
        self.gx, self.gn, self.hcol, self.hmom, self.rg = gx, gn, hcol, mom, dtr.raygen9(rg).copy()
        self.has = True
        self.dt_gen, self.dt_eye = self.geo_gen, np.asarray(eye, np.float32).reshape(3).copy()
        if self.on:
            self.dt_dirty = True
        self.followed = followed
        self.coords, self.lookup, self.diag = scratch[:2 * n].reshape(n, 2).copy(), scratch[2 * n:].reshape(n, 6).copy(), diag
        self.words = gn[:, 3].view(np.uint32).copy()
        return out, mom
