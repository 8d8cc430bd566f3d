"""csrc/bvh_fragment.h on the CPU: the clip that carries barycentric coordinates leaves the build's fragments as they were, and
the boxes the refit derives from those coordinates cover the moved triangle.

The header is RT_HD, so `g++ -ffp-contract=off` compiles the expressions hipcc compiles (as tests/denoise_ref.py does for the
denoiser). The program below holds, beside thin wrappers of the header, a VERBATIM restatement of the clip and the split loop
the device build had before the header existed (DevPoly / dpoly_clip / the loop of k_split_refs); the coverage check is numpy
float64 and shares no code with the header.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "bvh_fragment.h"

/* ---- the build's clip and split loop as they were (bvh_build_device.h before bvh_fragment.h), restated verbatim ---- */
struct DevPoly
{
    int n;
    float v[12][3];
};
static void dpoly_bounds(const DevPoly& p, float* lo, float* hi)
{
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int i = 0; i < p.n; ++i)
        for (int a = 0; a < 3; ++a)
        {
            lo[a] = fminf(lo[a], p.v[i][a]);
            hi[a] = fmaxf(hi[a], p.v[i][a]);
        }
}
static void dpoly_clip(const DevPoly& p, int a, float s, int sign, DevPoly& o)
{
    o.n = 0;
    for (int i = 0; i < p.n; ++i)
    {
        const float* c = p.v[i];
        const float* d = p.v[(i + 1) % p.n];
        const bool cin = sign > 0 ? c[a] >= s : c[a] <= s;
        const bool din = sign > 0 ? d[a] >= s : d[a] <= s;
        if (cin && o.n < 12) { o.v[o.n][0] = c[0]; o.v[o.n][1] = c[1]; o.v[o.n][2] = c[2]; o.n++; }
        if (cin != din && o.n < 12)
        {
            const float t = (s - c[a]) / (d[a] - c[a]);
            for (int k = 0; k < 3; ++k) o.v[o.n][k] = c[k] + (d[k] - c[k]) * t;
            o.v[o.n][a] = s;
            o.n++;
        }
    }
}
constexpr int SPLIT_STACK = 20;
extern "C" uint32_t frag_old(const float* t, float L, float* boxes, uint32_t cap, int* max_sp)
{
    DevPoly stack[SPLIT_STACK];
    int sp = 0;
    {
        stack[0].n = 3;
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) stack[0].v[k][a] = t[3 * k + a];
        sp = 1;
    }
    uint32_t emitted = 0;
    *max_sp = 1;
    while (sp > 0)
    {
        const DevPoly q = stack[--sp];
        float lo[3], hi[3];
        dpoly_bounds(q, lo, hi);
        int a = 0;
        for (int k = 1; k < 3; ++k)
            if (hi[k] - lo[k] > hi[a] - lo[a]) a = k;
        const float ext = hi[a] - lo[a];
        bool split = L > 0.0f && ext > L && emitted + (uint32_t)sp < 4096u && q.n >= 3 && sp + 2 <= SPLIT_STACK;
        float s = 0.0f;
        if (split)
        {
            const float mid = 0.5f * (lo[a] + hi[a]);
            s = L * floorf(mid / L + 0.5f);
            if (!(s > lo[a] + 0.01f * ext && s < hi[a] - 0.01f * ext)) s = mid;
            if (!(s > lo[a] && s < hi[a])) split = false;
        }
        if (split)
        {
            DevPoly l, r;
            dpoly_clip(q, a, s, -1, l);
            dpoly_clip(q, a, s, +1, r);
            if (l.n >= 3 && r.n >= 3)
            {
                stack[sp++] = l;
                stack[sp++] = r;
                if (sp > *max_sp) *max_sp = sp;
                continue;
            }
        }
        if (emitted < cap)
        {
            float* b = boxes + 6 * (size_t)emitted;
            for (int k = 0; k < 3; ++k) { b[k] = lo[k]; b[3 + k] = hi[k]; }
        }
        ++emitted;
    }
    return emitted;
}

/* ---- the header ---- */
extern "C" uint32_t frag_new(const float* t, float L, float* boxes, uint32_t cap)
{
    return rt::frag_split<false>(t, L, [&](uint32_t j, const rt::FragPoly<false>&, const float* lo, const float* hi) {
        if (j < cap) for (int k = 0; k < 3; ++k) { boxes[6 * (size_t)j + k] = lo[k]; boxes[6 * (size_t)j + 3 + k] = hi[k]; }
    });
}
/* with (u, v): boxes, vertex counts, uv[j][12][2] and positions pos[j][12][3] */
extern "C" uint32_t frag_new_uv(const float* t, float L, float* boxes, int* n, float* uv, float* pos, uint32_t cap)
{
    return rt::frag_split<true>(t, L, [&](uint32_t j, const rt::FragPoly<true>& q, const float* lo, const float* hi) {
        if (j >= cap) return;
        for (int k = 0; k < 3; ++k) { boxes[6 * (size_t)j + k] = lo[k]; boxes[6 * (size_t)j + 3 + k] = hi[k]; }
        n[j] = q.n;
        for (int i = 0; i < q.n; ++i)
        {
            uv[(j * 12 + i) * 2] = q.uv[i][0]; uv[(j * 12 + i) * 2 + 1] = q.uv[i][1];
            for (int k = 0; k < 3; ++k) pos[(j * 12 + i) * 3 + k] = q.v[i][k];
        }
    });
}
/* the refit's boxes (binary32) of m fragments under new vertices; uv as frag_new_uv wrote it */
extern "C" void frag_boxes(const float* tri, const float* uv, const int* n, uint32_t m, float* boxes)
{
    for (uint32_t j = 0; j < m; ++j) rt::frag_box(tri, tri + 3, tri + 6, uv + (size_t)j * 24, n[j], 2, boxes + 6 * (size_t)j, boxes + 6 * (size_t)j + 3);
}
static_assert(sizeof(rt::FragPoly<false>) == sizeof(DevPoly), "the build's polygons keep their size");
static_assert(rt::FRAG_SPLIT_STACK == SPLIT_STACK && rt::FRAG_MAX_VERTS == 12 && rt::FRAG_MAX_PER_TRI == 4096u, "caps");
"""

CAP = 4096 + 32
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="frag_ref_")
        src, so = os.path.join(d, "frag_ref.cpp"), os.path.join(d, "frag_ref.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        L.frag_old.argtypes, L.frag_old.restype = [vp, f32, vp, u32, vp], u32
        L.frag_new.argtypes, L.frag_new.restype = [vp, f32, vp, u32], u32
        L.frag_new_uv.argtypes, L.frag_new_uv.restype = [vp, f32, vp, vp, vp, vp, u32], u32
        L.frag_boxes.argtypes, L.frag_boxes.restype = [vp, vp, vp, u32, vp], None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data


_BUF = {}


def _buf(name, shape, dtype):
    """output buffers are reused (every caller slices [:count] and the next call of the same kind overwrites them)"""
    if name not in _BUF:
        _BUF[name] = np.zeros(shape, dtype)
    return _BUF[name]


def split_old(tri, L):
    boxes, sp = _buf("old", (CAP, 6), np.float32), C.c_int()
    m = lib().frag_old(_p(tri), L, _p(boxes), CAP, C.byref(sp))
    assert m <= CAP
    return boxes[:m], sp.value


def split_new(tri, L):
    boxes = _buf("new", (CAP, 6), np.float32)
    m = lib().frag_new(_p(tri), L, _p(boxes), CAP)
    assert m <= CAP
    return boxes[:m]


def split_uv(tri, L):
    boxes, n = _buf("uvb", (CAP, 6), np.float32), _buf("uvn", CAP, np.int32)
    uv, pos = _buf("uv", (CAP, 12, 2), np.float32), _buf("pos", (CAP, 12, 3), np.float32)
    m = lib().frag_new_uv(_p(tri), L, _p(boxes), _p(n), _p(uv), _p(pos), CAP)
    assert m <= CAP
    return boxes[:m], n[:m], uv[:m], pos[:m]


def refit_boxes(tri, uv, n):
    out = np.zeros((len(n), 6), np.float32)
    lib().frag_boxes(_p(np.ascontiguousarray(tri, np.float32)), _p(np.ascontiguousarray(uv)), _p(np.ascontiguousarray(n)), len(n), _p(out))
    return out


def _soup_vertices(seed, n):
    """the vertices of test_gpu_scene_update._soup: random triangles in a 10-unit cube, a tenth degenerate (a repeated vertex,
    three collinear vertices), with a few much larger ones so that several fragment lengths cut something"""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3), dtype=np.float32) * 10 - 5
    size = np.where(rng.random(n) < 0.1, 4.0, 0.6).astype(np.float32)[:, None, None]
    v = (c + rng.normal(size=(n, 3, 3)).astype(np.float32) * size).astype(np.float32)
    d = rng.random(n) < 0.05
    v[d, 1] = v[d, 0]
    col = (rng.random(n) < 0.05) & ~d
    v[col, 2] = (v[col, 0] + (v[col, 1] - v[col, 0]) * np.float32(2.0)).astype(np.float32)
    return np.ascontiguousarray(v.reshape(n, 9))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_clip_that_carries_uv_leaves_the_build_unchanged():
    """3000 triangles x 5 fragment lengths (0 = no pre-split): the header's split, with and without (u, v), gives the
    fragments of the restated old loop: same count, same order, boxes bit for bit. With (u, v), every vertex position is
    where its coordinates say (to rounding), and corners carry exactly (0,0), (1,0), (0,1)."""
    tris = _soup_vertices(7, 3000)
    split_some = 0
    for L in (0.0, 0.15, 0.5, 1.25, 3.0):
        for t in tris:
            old, _ = split_old(t, L)
            new = split_new(t, L)
            bx, n, uv, pos = split_uv(t, L)
            assert len(old) == len(new) == len(bx), (L, t)
            assert np.array_equal(_bits(old), _bits(new)), (L, t)
            assert np.array_equal(_bits(old), _bits(bx)), (L, t)
            if L == 0.0:
                assert len(old) == 1
            if len(old) > 1:
                split_some += 1
                A, B, Cv = (t[0:3].astype(np.float64), t[3:6].astype(np.float64), t[6:9].astype(np.float64))
                u, v = uv[..., 0].astype(np.float64)[..., None], uv[..., 1].astype(np.float64)[..., None]
                img = (1 - u - v) * A + u * B + v * Cv
                live = np.arange(12)[None, :] < n[:, None]
                scale = max(1.0, float(np.abs(t).max()))
                assert np.abs(img - pos)[live].max() < 2e-5 * scale, (L, t)
    assert split_some > 1000


# ---- coverage ----
def _lattice(N):
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    keep = i + j <= N
    return (i[keep] / N).astype(np.float64), (j[keep] / N).astype(np.float64)


def _needed_expansion(points, boxes):
    """per point: the smallest expansion (same on every side) of some box that makes it contain the point; float64"""
    best = np.full(len(points), np.inf)
    b = boxes.astype(np.float64)
    for s in range(0, len(b), 256):
        lo, hi = b[None, s:s + 256, 0:3], b[None, s:s + 256, 3:6]
        p = points[:, None, :]
        out = np.maximum(np.maximum(lo - p, p - hi), 0.0).max(axis=2)  # points x boxes
        best = np.minimum(best, out.min(axis=1))
    return best


def _coverage_slack(tri_build, L, tri_new, N=64, vertex_step=1):
    """split tri_build, move it to tri_new; returns (fragments, pad - the largest expansion any sampled point of the new
    triangle needs, pad). pad is the smallest the refit can use: 4e-5 * max(1, largest |coordinate| of the new triangle)."""
    _, n, uv, _ = split_uv(np.ascontiguousarray(tri_build, np.float32), L)
    new = np.ascontiguousarray(tri_new, np.float32)
    boxes = refit_boxes(new, uv, n)  # binary32, as the refit evaluates them
    A, B, Cv = (new[0:3].astype(np.float64), new[3:6].astype(np.float64), new[6:9].astype(np.float64))
    u, v = _lattice(N)
    fu = np.concatenate([uv[j, : n[j], 0] for j in range(0, len(n), vertex_step)]).astype(np.float64)
    fv = np.concatenate([uv[j, : n[j], 1] for j in range(0, len(n), vertex_step)]).astype(np.float64)
    u, v = np.concatenate([u, fu]), np.concatenate([v, fv])
    pts = (1 - u - v)[:, None] * A + u[:, None] * B + v[:, None] * Cv
    pad = 4e-5 * max(1.0, float(np.abs(new).max()))
    need = _needed_expansion(pts, boxes)
    return len(n), pad - float(need.max()), pad


def _rot90x(t):
    v = t.reshape(3, 3).astype(np.float32)
    return np.stack([v[:, 0], -v[:, 2], v[:, 1]], 1).astype(np.float32).reshape(9)


BIG = np.float32([-3.7, 0.3, -2.9, 4.1, 0.9, -1.3, 0.6, -0.4, 4.4])          # a generic large triangle
FLOOR = np.float32([-8, 0, -8, 8, 0, -8, 8, 0, 8])                           # axis-aligned: vertices on grid lines
COLLINEAR = np.float32([-4, 1, -3, 0, 1.5, -1, 4, 2, 1])                     # C = A + 2 (B - A)
REPEATED = np.float32([-4, 1, -3, -4, 1, -3, 4, 2, 3])                       # A == B


def _updates_of(t):
    v = t.reshape(3, 3)
    return [
        ("identity", t),
        ("rigid move", (v + np.float32([0.5, 0.0, 0.25])).astype(np.float32).reshape(9)),
        ("rotated 90 degrees about x", _rot90x(t)),
        ("scaled 100x", (t * np.float32(100.0)).astype(np.float32)),
        ("mirrored", (v * np.float32([-1, 1, 1])).astype(np.float32).reshape(9)),
        ("collapsed to a segment", np.concatenate([v[0], v[1], ((v[0] + v[1]) * np.float32(0.5)).astype(np.float32)])),
        ("collapsed to a point", np.concatenate([v[0], v[0], v[0]])),
        ("sheared far away", np.concatenate([v[0] + np.float32(900.0), v[1] - np.float32(350.0), v[2]]).astype(np.float32)),
    ]


def test_refitted_fragment_boxes_cover_the_moved_triangle():
    """Every sampled point of the new triangle (a 64-step barycentric lattice and the image of every fragment vertex) lies in
    the box of at least one fragment expanded by LESS than the pad. Reported: the smallest slack (pad - expansion needed)
    relative to the pad; 1.0 = no expansion needed at all."""
    worst = (np.inf, None)
    for name, t, L in (("big", BIG, 0.5), ("big, L not a grid the vertices know", BIG, 0.37), ("floor", FLOOR, 1.0)):
        for label, new in _updates_of(t):
            m, slack, pad = _coverage_slack(t, L, new)
            assert m > 50, (name, m)
            assert slack > 0.0, f"{name}: {label}: a point needs {pad - slack:.3e} of a pad of {pad:.3e}"
            worst = min(worst, (slack / pad, f"{name}: {label}"))
    # degenerate at build (still split: an extent exceeds L), made large and proper by the update
    for name, t in (("collinear", COLLINEAR), ("repeated vertex", REPEATED)):
        for label, new in (("made a large triangle", np.float32([-40, 3, -30, 35, -8, -12, 2, 60, 44])), ("rigid move", (t.reshape(3, 3) + np.float32([0.5, 0, 0.25])).astype(np.float32).reshape(9)),
                           ("rotated", _rot90x(t))):
            m, slack, pad = _coverage_slack(t, 0.5, new)
            assert m >= 8, (name, m)
            assert slack > 0.0, f"{name}: {label}: a point needs {pad - slack:.3e} of a pad of {pad:.3e}"
            worst = min(worst, (slack / pad, f"{name}: {label}"))
    print(f"smallest slack / pad = {worst[0]:.4f} ({worst[1]})")
    assert worst[0] > 0.5  # the argument of bvh_fragment.h leaves at least 45 % of the pad unused; far more in practice


def test_fragment_caps():
    """A triangle that reaches the 4096-fragment cap and a sliver whose split recursion fills the stack: the build is still
    unchanged, and the fragments still cover the triangle after an update."""
    wide = np.float32([-60, 0.1, -55, 58, 0.4, -50, 3, -0.2, 61])
    old, _ = split_old(wide, 0.5)
    old = old.copy()
    assert 4096 <= len(old) <= 4096 + 20, len(old)
    sliver = np.float32([0, 0, 0, 3.0e6, 1, 0.5, 3.0e6, 1.5, 0.25])
    old_s, max_sp = split_old(sliver, 1.0)
    old_s = old_s.copy()
    assert max_sp == 20, max_sp
    for t, L, o in ((wide, 0.5, old), (sliver, 1.0, old_s)):
        new = split_new(t, L)
        bx, n, uv, pos = split_uv(t, L)
        assert len(new) == len(bx) == len(o)
        assert np.array_equal(_bits(o), _bits(new)) and np.array_equal(_bits(o), _bits(bx))
        assert n.max() <= 12 and n.min() >= 3
        for label, upd in (("rotated", _rot90x(t)),
                           ("small and elsewhere", (t * np.float32(0.001) + np.float32(7.0)).astype(np.float32))):
            m, slack, pad = _coverage_slack(t, L, upd, N=32, vertex_step=8)
            assert slack > 0.0, f"{label}: a point needs {pad - slack:.3e} of a pad of {pad:.3e}"
