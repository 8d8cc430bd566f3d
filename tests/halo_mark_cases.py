"""The cases of the halo-mark tests and their reference, shared by tests/test_halo_ref_cpu.py (the reference alone: it must
exercise what the cases claim) and tests/test_gpu_halo_kernels.py (rt_halo_mark[_sides] against it).

Reference: the oracle's spatial loop itself (oracle.binding.Scene.spatial_reads), run over the strip's own rows on the oracle's
G-buffer; the neighbours' flags enter as the `index` of the halo rows' visibility records. Nothing here reads csrc/."""
import numpy as np

import halo_ref

EYE, AT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)
FOVY = np.float32(np.pi) / np.float32(4)
FRAMES = (1, 2, 1000003)
FLAG_KINDS = ("real", "random", "zero", "one", "checker")

# name -> W, H, own rows, halo, option overrides, (first_pass, n_passes) calls
CASES = {
    "M1": (64, 270, (90, 180), 87, {}, [(0, 3)]),
    "M2": (100, 270, (90, 180), 87, {}, [(0, 3)]),
    "M3lo": (64, 270, (0, 90), 87, {}, [(0, 3)]),
    "M3hi": (64, 270, (180, 270), 87, {}, [(0, 3)]),
    "M4": (32, 400, (100, 300), 87, {}, [(0, 3)]),
    "M5": (37, 120, (40, 80), 29, dict(spatial_resampling_radius=10.0), [(0, 3)]),
    "M6": (64, 270, (90, 180), 87, dict(spatial_resampling_passes=5), [(0, 5), (0, 4), (1, 2), (2, 1), (0, 3)]),
    "M7n9": (64, 270, (90, 180), 87, dict(spatial_resampling_sample_count=9), [(0, 3)]),
    "M7n1": (64, 270, (90, 180), 87, dict(spatial_resampling_sample_count=1), [(0, 3)]),
    "M7off": (64, 270, (90, 180), 87, dict(use_spatial_resampling=0), [(0, 3)]),
}
FULL = ("M1", "M2")  # every flags pattern, every frame, every tuning
# fewest marks per side and pass under the real flags (the issue's floors; measured on the oracle: see docs/MEASUREMENT_LOG_r26.md)
MIN_MARKS = {"M1": 200, "M2": 200, "M3lo": 200, "M3hi": 200, "M4": 200, "M5": 100, "M6": 200, "M7n9": 200, "M7n1": 100, "M7off": 0}

_vis_cache = {}
_ref_cache = {}


def flag_bytes(ob, sc, vis):
    """1 on a shaded pixel, 2 on an emissive one, 0 on sky"""
    idx = vis["index"]
    emissive = (idx >= 0) & np.isin(idx, sc.lights.astype(np.int64))
    return np.where(idx < 0, 0, np.where(emissive, 2, 1)).astype(np.uint8)


class Reference:
    """One case on the oracle: flags(kind) per side, picks(kind, frame, pass) = (touched, read) of the strip's own rows,
    expected(kind, frame, first_pass, n_passes) = the word arrays the device must produce per side."""

    def __init__(self, ob, name):
        from cedec_2024_rt_amd import scenes

        self.ob, self.name = ob, name
        self.W, self.H, self.rows, self.halo, self.optkw, self.calls = CASES[name]
        W, H, (a, b), halo = self.W, self.H, self.rows, self.halo
        self.tris = scenes.make_quad_room()
        self.opt = ob.bench_options(**self.optkw)
        self.count = int(self.opt["spatial_resampling_sample_count"][0])
        self.passes = int(self.opt["spatial_resampling_passes"][0])
        ob.set_math_mode(ob.MATH_PORTABLE)
        self.sc = ob.Scene(self.tris, use_bvh=True)
        self.rg = ob.raygen_lookat(EYE, AT, (0, 1, 0), FOVY, W, H)
        if (W, H) not in _vis_cache:
            _vis_cache[(W, H)] = self.sc.raycast(W, H, self.rg)
        self.vis = _vis_cache[(W, H)]
        self.real = flag_bytes(ob, self.sc, self.vis)
        self.plain_triangle = int(np.setdiff1d(np.arange(len(self.tris)), self.sc.lights.astype(np.int64))[0])
        self.held = (max(0, a - halo), min(H, b + halo))
        self.regions = {}  # side -> (row0, rows)
        if a > 0:
            self.regions[0] = (self.held[0], a - self.held[0])
        if b < H:
            self.regions[1] = (b, self.held[1] - b)
        self._picks = {}

    def flags(self, kind):
        """side -> uint8 (rows * W) of the neighbour's flags"""
        out = {}
        for side, (r0, n) in self.regions.items():
            if kind == "real":
                f = self.real[r0 * self.W:(r0 + n) * self.W].copy()
            elif kind == "random":
                f = np.random.default_rng([17, side, self.W, self.H]).integers(0, 3, n * self.W).astype(np.uint8)
            elif kind == "zero":
                f = np.zeros(n * self.W, np.uint8)
            elif kind == "one":
                f = np.ones(n * self.W, np.uint8)
            elif kind == "checker":
                yy, xx = np.mgrid[r0:r0 + n, 0:self.W]
                f = ((xx + yy) & 1).astype(np.uint8).ravel()
            else:
                raise KeyError(kind)
            out[side] = f
        return out

    def vis_for(self, kind):
        if kind == "real":
            return self.vis
        vis = self.vis.copy()
        for side, f in self.flags(kind).items():
            r0, n = self.regions[side]
            vis["index"][r0 * self.W:(r0 + n) * self.W] = np.where(f & 1, self.plain_triangle, -1)
        return vis

    def picks(self, kind, frame, pas):
        key = (kind, frame, pas)
        if key not in self._picks:
            self.ob.set_math_mode(self.ob.MATH_PORTABLE)
            rin = np.zeros(self.W * self.H, dtype=self.ob.RESERVOIR)
            _, touched, read = self.sc.spatial_reads(self.W, self.H, frame, pas, self.vis_for(kind), np.asarray(EYE, np.float32), self.opt, rin,
                                                     rows=self.rows)
            self._picks[key] = (touched, read)
        return self._picks[key]

    def bits(self, kind, frame, pas, side, which=0):
        r0, n = self.regions[side]
        return halo_ref.region_bits(self.picks(kind, frame, pas)[which], self.W, self.rows, r0, n)

    def expected(self, kind, frame, first_pass, n_passes):
        out = {}
        for side, (r0, n) in self.regions.items():
            out[side] = np.concatenate([halo_ref.need_bitmaps(self.picks(kind, frame, p)[0], self.W, self.rows, r0, n)
                                        for p in range(first_pass, first_pass + n_passes)])
        return out

    def rows_outside_held(self, kind, frame, pas):
        t = self.picks(kind, frame, pas)[0]
        t = t[t >= 0] // self.W
        return int(((t < self.held[0]) | (t >= self.held[1])).sum())


def reference(ob, name):
    if name not in _ref_cache:
        _ref_cache[name] = Reference(ob, name)
    return _ref_cache[name]
