"""Rays aimed AT the geometry, for the claim "the BVH walk equals brute force" (csrc/bvh_cull.h).

A uniformly random ray never passes within a few ulps of a box face, which is the only place a cull can be wrong. These do:
every ray is aimed at a vertex, at a point of an edge or at an interior point of a triangle, a quarter of them end at the
target (the range edge), and extra rays start in box face planes or run along shared tile edges. Helper only: the tests are
tests/test_targeted_rays_cpu.py and tests/test_gpu_targeted_rays.py. Everything is generated from seeds.
"""
import numpy as np

from cedec_2024_rt_amd.types import TRIANGLE

DISTS = (3.0, 30.0, 1000.0)
N_RAYS = 200000
VERTEX, EDGE, INTERIOR, EXTRA = 0, 1, 2, 3
F32_MAX = np.float32(3.0e38)


def make_tris(v):
    t = np.zeros(len(v), TRIANGLE)
    t["v"] = np.asarray(v, np.float32).reshape(-1, 3, 3)
    t["color"] = 0.5
    return t


def _quad(p, a, b):
    """two triangles of the parallelogram p, p + a, p + a + b, p + b"""
    p, a, b = (np.asarray(x, np.float32) for x in (p, a, b))
    return [[p, p + a, p + a + b], [p, p + a + b, p + b]]


def floor_tiles(n=8):
    v = []
    for z in range(n):
        for x in range(n):
            v += _quad((x, 0, z), (1, 0, 0), (0, 0, 1))
    return np.asarray(v, np.float32)


def walls(n=8, h=4):
    v = _quad((0, 0, 0), (n, 0, 0), (0, h, 0)) + _quad((0, 0, n), (n, 0, 0), (0, h, 0))
    v += _quad((0, 0, 0), (0, 0, n), (0, h, 0)) + _quad((n, 0, 0), (0, 0, n), (0, h, 0))
    return np.asarray(v, np.float32)


def soup(n=300, seed=77):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3)) * 1.5
    return (c + rng.normal(size=(n, 3, 3)) * 0.8).astype(np.float32)


def scene_vertices():
    """name -> (n, 3, 3) float32 vertices; every scene has at most 600 triangles"""
    a = floor_tiles()
    b = np.concatenate([a, walls()])
    c = soup()
    s = {"a_tiles": a, "b_tiles_walls": b, "c_soup": c,
         "d_soup_1e3": (c + np.float32(1000.0)).astype(np.float32), "d_soup_1e5": (c + np.float32(1.0e5)).astype(np.float32)}
    for k in list(s):
        s["e_twice_" + k] = np.concatenate([s[k], s[k]])
    s["f_tiles_2^-10"] = (a * np.float32(2.0 ** -10)).astype(np.float32)
    s["f_tiles_2^10"] = (a * np.float32(2.0 ** 10)).astype(np.float32)
    s["g_tiles_shifted"] = (a + np.float32([0.1, 0.3, 0.7])).astype(np.float32)
    assert all(len(v) <= 600 for v in s.values())
    return s


SCENES = scene_vertices()
DOUBLED = {k: len(v) // 2 for k, v in SCENES.items() if k.startswith("e_twice_")}


def targeted(tri_v, rng, n, dist, graze):
    """(rays (n, 8) float32 = origin, direction, tmin, tmax; kind (n,); target triangle (n,))"""
    f = np.float32
    tri = rng.integers(0, len(tri_v), n)
    kind = (np.arange(n) % 3).astype(np.int32)
    r = rng.random(n, dtype=np.float32)
    sel = rng.integers(0, 3, n)
    w0, w1 = np.zeros(n, f), np.zeros(n, f)
    # vertices: weights exactly 0 and 1
    m = kind == VERTEX
    w0[m & (sel == 1)] = 1.0
    w1[m & (sel == 2)] = 1.0
    # edges: one weight exactly 0 (for sel == 2 it is 1 - w0 - w1: (1 - w0) - w1 == 0 in binary32)
    m = kind == EDGE
    w0[m & (sel == 0)] = r[m & (sel == 0)]
    w1[m & (sel == 1)] = r[m & (sel == 1)]
    w0[m & (sel == 2)] = r[m & (sel == 2)]
    w1[m & (sel == 2)] = (f(1.0) - r[m & (sel == 2)]).astype(f)
    m = kind == INTERIOR
    a, b = r[m], rng.random(int(m.sum()), dtype=np.float32)
    flip = a + b > 1
    w0[m] = np.where(flip, 1 - a, a).astype(f) * f(0.98) + f(0.01)
    w1[m] = np.where(flip, 1 - b, b).astype(f) * f(0.98)
    v = tri_v[tri]
    w2 = ((f(1.0) - w0) - w1).astype(f)
    target = ((w2[:, None] * v[:, 0] + w0[:, None] * v[:, 1]).astype(f) + w1[:, None] * v[:, 2]).astype(f)
    off = (f(dist) * rng.normal(size=(n, 3)).astype(f)).astype(f)
    if graze:
        off[1::2, 1] = np.abs(off[1::2, 1]) * f(0.01)
    origin = (target + off).astype(f)
    factor = np.where(rng.integers(0, 2, n) == 0, f(1.0), f(1.5)).astype(f)
    rays = np.zeros((n, 8), f)
    rays[:, 0:3] = origin
    rays[:, 3:6] = ((target - origin).astype(f) * factor[:, None]).astype(f)
    rays[:, 7] = F32_MAX
    rays[3::4, 7] = 0.99  # factor 1.5: the target lies inside [0, 0.99]; factor 1.0: just outside, the range edge
    return rays, kind, tri


def face_plane_rays(tri_v, rng, n):
    """rays that start exactly in a box face plane (an origin coordinate equal to a vertex coordinate) whose direction component
    on that axis is 1e-3, 1e-6 or 0 of the largest other one; aimed at points of triangles otherwise"""
    f = np.float32
    base, _, _ = targeted(tri_v, rng, n, 3.0, False)
    axis = rng.integers(0, 3, n)
    vert = tri_v.reshape(-1, 3)[rng.integers(0, 3 * len(tri_v), n)]
    idx = np.arange(n)
    base[idx, axis] = vert[idx, axis]
    other = np.abs(base[:, 3:6]).copy()
    other[idx, axis] = 0
    frac = np.asarray([1e-3, 1e-6, 0.0], f)[rng.integers(0, 3, n)]
    sign = np.where(rng.integers(0, 2, n) == 0, f(-1), f(1))
    base[idx, 3 + axis] = (other.max(axis=1) * frac * sign).astype(f)
    base[:, 7] = F32_MAX
    return base


def seam_rays(tri_v, rng, n):
    """rays aimed exactly along a triangle edge (for the tiles: a shared seam): half of them run inside the edge's line, half
    start straight above a point of the edge's line and come down on it within the plane that holds the edge and the offset"""
    f = np.float32
    tri = rng.integers(0, len(tri_v), n)
    e = rng.integers(0, 3, n)
    a, b = tri_v[tri, e], tri_v[tri, (e + 1) % 3]
    d = (b - a).astype(f)
    k = rng.integers(1, 4, n).astype(f)
    rays = np.zeros((n, 8), f)
    rays[:, 0:3] = (a - d * k[:, None]).astype(f)
    rays[:, 3:6] = d
    up = np.zeros((n, 3), f)
    up[:, 1] = rng.integers(1, 4, n)
    rays[1::2, 0:3] = (rays[1::2, 0:3] + up[1::2]).astype(f)
    rays[1::2, 3:6] = (d[1::2] * (k[1::2, None] + rng.random((n, 1), dtype=np.float32)[1::2]) - up[1::2]).astype(f)
    rays[:, 7] = F32_MAX
    return rays


N_EXTRA = 6000

_RAYS = {}
_REF = {}


def rays_for(name, dist, tri_v=None, seed_salt=0):
    """the ray set of one (scene, dist): N_RAYS targeted rays (grazing ones on the flat scenes) followed by N_EXTRA face-plane and
    seam rays. Cached; callers must not write into it. tri_v: other vertices for the same recipe (moved geometry)."""
    key = (name, dist, seed_salt)
    if key not in _RAYS:
        v = SCENES[name] if tri_v is None else tri_v
        rng = np.random.default_rng([sorted(SCENES).index(name), int(dist), seed_salt])
        rays, kind, tri = targeted(v, rng, N_RAYS, dist, graze=not ("soup" in name))
        extra = np.concatenate([face_plane_rays(v, rng, N_EXTRA // 2), seam_rays(v, rng, N_EXTRA // 2)])
        _RAYS[key] = (np.ascontiguousarray(np.concatenate([rays, extra])), np.concatenate([kind, np.full(N_EXTRA, EXTRA, np.int32)]),
                      np.concatenate([tri, np.full(N_EXTRA, -1)]))
    return _RAYS[key]


def brute_force(oracle, tri_v, rays):
    return oracle.Scene(make_tris(tri_v), use_bvh=False).trace_closest(rays, force_brute=True)


def reference(oracle, name, dist):
    """(rays, kind, brute-force hits (n, 4) float32 = t, u, v, bits(index)) of one (scene, dist), computed once per process; the
    conditions that make the case worth running are asserted here, on the reference alone"""
    key = (name, dist)
    if key not in _REF:
        rays, kind, _ = rays_for(name, dist)
        ref = brute_force(oracle, SCENES[name], rays)
        hit = ref[:, 3].view(np.int32) >= 0
        assert hit[:N_RAYS].mean() >= 0.8, f"{name} dist {dist}: only {hit[:N_RAYS].mean():.3f} of the targeted rays hit"
        nv, ne = int((hit & (kind == VERTEX)).sum()), int((hit & (kind == EDGE)).sum())
        assert nv >= 10000 and ne >= 10000, f"{name} dist {dist}: {nv} reference hits at vertices, {ne} on edges"
        if name in DOUBLED:  # every triangle twice: at equal t the later copy wins
            assert (ref[hit, 3].view(np.int32) >= DOUBLED[name]).all(), f"{name}: brute force reports a first-copy winner"
        ref.setflags(write=False)
        _REF[key] = (rays, kind, ref)
    return _REF[key]
