"""Scenes and rays for the device BVH build (csrc/bvh_build_device.h): sizes on the borders of its three regimes (small subtrees
of at most 64 references, medium nodes of 65..4096, large nodes above), forced first splits that land the children on those
borders, centroid distributions that take the binning's degenerate paths, and the pre-split budget scene. Helper only: the
tests are tests/test_gpu_bvh_build.py (device) and tests/test_bvh_build_scenes_cpu.py (the conditions on the reference alone).
Pure numpy, everything from seeds; a centroid below is what the builders bin: the centre 0.5 * (lo + hi) of a reference's box.
"""
import numpy as np

import targeted_rays as T

N_RAYS = 4096  # per scene: half random, half aimed at vertices and edge points
SAH_SMALL, SAH_MEDIUM = 64, 4096
REGIME_SIZES = (2, 3, 4, 5, 63, 64, 65, 66, 4095, 4096, 4097, 4098)
CLUSTER_SIZES = ((64, 65), (1, 65), (4096, 4097), (64, 4097))
DEGENERATE_SIZES = (40, 1000, 6000)  # one per regime
DEGENERATE_KINDS = ("a_copies", "b_concentric", "c_line", "d_plane", "e_far_clusters", "f_enclosed")
MIN_HIT_FRACTION = 0.2


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def soup(n, seed, size=0.5):
    """n triangles from continuous distributions: centres uniform in +-half, vertices normal(size) around them; no duplicates.
    half grows with the cube root of n up to 4, so that random rays through the scene's box hit something at every size"""
    rng = np.random.default_rng([1801, seed, n])
    half = float(min(0.25 * n ** (1.0 / 3.0), 4.0))
    c = rng.uniform(-half, half, size=(n, 1, 3))
    return _f32(c + rng.normal(size=(n, 3, 3)) * size)


def soup_with_large(n, seed):
    """soup(n) with a few triangles scaled to 50 x the median extent about their centre: the default split factor cuts them"""
    v = soup(n, seed).astype(np.float64)
    ext = (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    k = max(1, min(4, n // 8))
    rng = np.random.default_rng([1802, seed, n])
    big = rng.choice(n, size=k, replace=False)
    for i in big:
        c = v[i].mean(axis=0)
        v[i] = c + (v[i] - c) * (50.0 * np.median(ext) / ext[i])
    return _f32(v)


def two_clusters(na, nb, seed):
    """two clusters of diameter 1 whose centres lie 100 apart on a skew line: every centroid of the first falls in bin 0 and
    every one of the second in bin 31 of the root, so the first split is na | nb whatever the SAH makes of the rest"""
    rng = np.random.default_rng([1803, seed, na, nb])
    d = np.asarray([0.8, 0.5, 0.33166247903554])  # unit length
    out = []
    for n, o in ((na, -50.0 * d), (nb, 50.0 * d)):
        c = rng.uniform(-0.4, 0.4, size=(n, 1, 3))
        out.append(o + c + rng.uniform(-0.1, 0.1, size=(n, 3, 3)))
    return _f32(np.concatenate(out))


def cluster_boxes(na, nb):
    d = np.asarray([0.8, 0.5, 0.33166247903554])
    return [(o - 0.55, o + 0.55) for o in (-50.0 * d, 50.0 * d)]


def _boxed_tris(rng, lo, hi):
    """one triangle per row whose box is exactly [lo, hi] (n, 3 each): per axis one vertex takes lo, another hi and the third
    a value between, in a random arrangement (random orientations)"""
    n = len(lo)
    v = np.zeros((n, 3, 3))
    for a in range(3):
        perm = np.argsort(rng.random((n, 3)), axis=1)
        mid = lo[:, a] + (hi[:, a] - lo[:, a]) * rng.uniform(0.1, 0.9, n)
        vals = np.stack([lo[:, a], hi[:, a], mid], axis=1)
        v[np.arange(n)[:, None], perm, a] = vals
    return v


def degenerate(kind, n, seed=0):
    """(vertices (n, 3, 3) float32, boxes the random rays start in, or None for the scene's bounds)

    a_copies        n copies of one triangle
    b_concentric    boxes symmetric about the origin (every centroid is exactly 0), half extents log-uniform over 3 decades
    c_line          centroids on the x axis: boxes symmetric in y and z, centre x uniform in +-10
    d_plane         centroids in the plane y = 0
    e_far_clusters  two clusters of extent 1, 1e6 apart (binary32 resolves 1/16 there): bins 0 and 31 only at the root
    f_enclosed      a cluster in the unit cube and one triangle of extent 1e4 whose box encloses it
    """
    rng = np.random.default_rng([1804, DEGENERATE_KINDS.index(kind), n, seed])
    boxes = None
    if kind == "a_copies":
        one = np.asarray([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.0, 0.5]])
        v = np.repeat(one[None], n, axis=0)
    elif kind in ("b_concentric", "c_line", "d_plane"):
        if kind == "b_concentric":
            h = (10.0 ** rng.uniform(-2.0, 1.0, size=(n, 1))) * rng.uniform(0.5, 1.0, size=(n, 3))
        else:
            h = rng.uniform(0.2, 0.8, size=(n, 3))
        h = _f32(h).astype(np.float64)  # lo = -h and hi = h exactly, also after the build's padding
        c = np.zeros((n, 3))
        if kind == "c_line":
            c[:, 0] = rng.uniform(-10.0, 10.0, n)
        if kind == "d_plane":
            c[:, 0] = rng.uniform(-6.0, 6.0, n)
            c[:, 2] = rng.uniform(-6.0, 6.0, n)
        v = _boxed_tris(rng, c - h, c + h)
        sym = {"b_concentric": (0, 1, 2), "c_line": (1, 2), "d_plane": (1,)}[kind]
        v32 = _f32(v)
        for a in sym:  # the symmetric axes are exact in binary32 (c = 0 there, h is binary32)
            assert (v32[:, :, a].min(axis=1) == -v32[:, :, a].max(axis=1)).all()
        if kind == "b_concentric":
            boxes = [(np.full(3, -1.0), np.full(3, 1.0))]
    elif kind == "e_far_clusters":
        na = n // 2
        parts = []
        boxes = []
        for m, o in ((na, np.zeros(3)), (n - na, np.asarray([1.0e6, 0.0, 0.0]))):
            c = rng.uniform(0.3, 0.7, size=(m, 1, 3))
            parts.append(o + c + rng.uniform(-0.3, 0.3, size=(m, 3, 3)))
            boxes.append((o, o + 1.0))
        v = np.concatenate(parts)
    elif kind == "f_enclosed":
        c = rng.uniform(0.1, 0.9, size=(n - 1, 1, 3))
        v = c + rng.uniform(-0.1, 0.1, size=(n - 1, 3, 3))
        big = np.asarray([[[-5000.0, -0.5, -5000.0], [5000.0, -0.25, -4000.0], [0.0, 1.5, 5000.0]]])
        v = np.concatenate([v, big])
        boxes = [(np.full(3, -0.5), np.full(3, 1.5))]
    else:
        raise KeyError(kind)
    return _f32(v), boxes


def budget_scene(n=2000, large=0.1, seed=0):
    """a tessellated object among large walls: centres uniform in +-20, a fraction `large` of the triangles with vertices spread
    +-10 about the centre, the rest +-1e-4. With split factor 10 the length that starts the pre-split is 10 x a tiny median"""
    rng = np.random.default_rng([1805, seed, n, int(round(large * 100))])
    c = rng.uniform(-20.0, 20.0, size=(n, 1, 3))
    spread = np.where(rng.random(n) < large, 10.0, 1.0e-4)[:, None, None]
    return _f32(c + rng.uniform(-1.0, 1.0, size=(n, 3, 3)) * spread)


def equal_size_scene(n=500, seed=0):
    """every triangle the same size: the first length fits"""
    rng = np.random.default_rng([1806, seed, n])
    c = rng.uniform(-20.0, 20.0, size=(n, 1, 3))
    return _f32(c + rng.uniform(-1.0, 1.0, size=(n, 3, 3)))


def split_length(v, factor):
    """the builders' first fragment length: factor x the median (element n // 2 of the sorted) largest box extent, in binary32"""
    v = _f32(v)
    ext = (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    return np.float32(factor) * np.sort(ext)[len(ext) // 2]


def random_rays(rng, n, boxes):
    """as test_gpu_parity._random_rays (origins uniform in a box, directions uniform in +-1, some axis-parallel, some short), the
    origins spread over `boxes` in turn"""
    f = np.float32
    rays = np.zeros((n, 8), f)
    for k, (lo, hi) in enumerate(boxes):
        lo, hi = _f32(lo), _f32(hi)
        m = len(rays[k::len(boxes)])
        rays[k::len(boxes), 0:3] = (rng.random((m, 3), dtype=f) * (hi - lo) + lo).astype(f)
    rays[:, 3:6] = (rng.random((n, 3), dtype=f) * 2 - 1).astype(f)
    rays[:, 7] = 3.402823466e38
    rays[: n // 16, 3] = 0.0
    rays[n // 16: n // 8, 4] = 0.0
    rays[n // 8: n // 4, 7] = 0.99
    return rays


def scene_rays(v, seed, boxes=None, dist=3.0):
    """N_RAYS rays: random ones, then targeted_rays' rays at vertices and at points of edges"""
    rng = np.random.default_rng([1807, seed, len(v)])
    if boxes is None:
        p = v.reshape(-1, 3)
        boxes = [(p.min(axis=0) - 0.1, p.max(axis=0) + 0.1)]
    half = N_RAYS // 2
    aimed, kind, _ = T.targeted(v, rng, 3 * half, dist, graze=False)
    aimed = aimed[kind != T.INTERIOR][:half]
    assert len(aimed) == half
    return np.ascontiguousarray(np.concatenate([random_rays(rng, N_RAYS - half, boxes), aimed]))


def _make(name):
    """name -> (vertices, ray boxes or None, split factor or None for the default)"""
    kind, _, rest = name.partition(":")
    if kind == "soup":
        return soup(int(rest), 1), None, 0.0
    if kind == "large":
        return soup_with_large(int(rest), 1), None, None
    if kind == "clusters":
        na, nb = (int(x) for x in rest.split("+"))
        return two_clusters(na, nb, 1), cluster_boxes(na, nb), 0.0
    if kind == "budget":
        return budget_scene(int(rest)), None, 10.0
    dk, _, n = rest.partition("@")
    v, boxes = degenerate(dk, int(n))
    return v, boxes, 0.0


SOUPS = tuple(f"soup:{n}" for n in REGIME_SIZES)
CLUSTERS = tuple(f"clusters:{a}+{b}" for a, b in CLUSTER_SIZES)
LARGE = tuple(f"large:{n}" for n in REGIME_SIZES)
DEGENERATE = tuple(f"degenerate:{k}@{n}" for k in DEGENERATE_KINDS for n in DEGENERATE_SIZES)
BUDGET = "budget:2000"
ALL = SOUPS + CLUSTERS + LARGE + DEGENERATE + (BUDGET,)

_SCENES = {}
_REF = {}


def scene(name):
    """(vertices, rays, split factor or None); cached, callers must not write into them"""
    if name not in _SCENES:
        v, boxes, split = _make(name)
        rays = scene_rays(v, ALL.index(name), boxes)
        v.setflags(write=False)
        rays.setflags(write=False)
        _SCENES[name] = (v, rays, split)
    return _SCENES[name]


def reference(oracle, name):
    """(vertices, rays, brute-force hits (n, 4) float32 = t, u, v, bits(index), split factor), computed once per process. At least
    a fifth of the rays hit: asserted here, on the reference alone"""
    if name not in _REF:
        v, rays, split = scene(name)
        ref = T.brute_force(oracle, v, rays)
        hit = ref[:, 3].view(np.int32) >= 0
        assert hit.mean() >= MIN_HIT_FRACTION, f"{name}: only {hit.mean():.3f} of the rays hit"
        ref.setflags(write=False)
        _REF[name] = (v, rays, ref, split)
    return _REF[name]
