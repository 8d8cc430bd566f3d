"""The indirect pass (rt_indirect) on the CPU: tests/indirect_ref.py, the restatement the GPU tests compare the
kernels with, is (1) anchored to the oracle's 08_nee through its CAMERA start, (2) shown to differ from that start only where the last
bits of the surface point send a bounce ray elsewhere, (3) unbiased against the oracle's own tail, and (4) exact at its edges.

Setup, as measured when the pass was specified: scenes.make_quad_room() (92 triangles), 64 x 48, eye (0.5, 3, 6) -> (0, 1, -1.5),
fovy 0.9 (the view of tests/test_restir_unbiased_cpu.py), 2 329 shaded pixels.
  (1) pixels with a tail > 0 at D = 2 / 3 / 6, frame 7: 400 / 435 / 440, 6.2 / 7.1 / 7.4 % of the frame's energy.
  (2) GBUFFER against CAMERA, bounces 5, frames 1-12: 1 of 27 948 paths differs by more than 1e-4 relative.
  (3) mean of R + G + B over the shaded pixels, 500 frames each side: ours 0.023923, the oracle's tail 0.024097, -1.73 SE of the
      difference, no pixel beyond |z| = 4 (max 3.81)."""
import numpy as np
import pytest

import indirect_ref as ir
from restir_unbiased_ref import LEDGE_AT, LEDGE_EYE, make_ledge
from test_restir_unbiased_cpu import _Seq, _compare

EYE, AT, FOVY = (0.5, 3.0, 6.0), (0.0, 1.0, -1.5), np.float32(0.9)
W, H = 64, 48


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _World:
    def __init__(self, oracle, tris, eye, at, w=W, h=H):
        oracle.set_math_mode(oracle.MATH_PORTABLE)
        self.o, self.tris, self.eye, self.W, self.H = oracle, tris, np.asarray(eye, np.float32), w, h
        self.scene = oracle.Scene(tris, use_bvh=True)
        self.rg = oracle.raygen_lookat(eye, at, (0, 1, 0), FOVY, w, h)
        self.vis = self.scene.raycast(w, h, self.rg)
        lit = (tris["emissive"] > 0).any(axis=1)
        self.sky = self.vis["index"] < 0
        self.emissive = ~self.sky & lit[np.maximum(self.vis["index"], 0)]
        self.shaded = ~self.sky & ~self.emissive

    def nee(self, frame, max_depth):
        """oracle path_trace(8) of one frame, accumulate = 0: (W * H, 3)"""
        acc = np.zeros((self.W * self.H, 4), np.float32)
        self.scene.path_trace(8, self.W, self.H, frame, self.rg, self.o.default_options(max_depth=max_depth), acc)
        return acc[:, :3].copy()

    def tail(self, frame, bounces, start=ir.GBUFFER):
        return ir.tail(self.W, self.H, frame, self.tris, self.vis, self.eye, self.rg, bounces, start)


@pytest.fixture(scope="module")
def room(oracle):
    from cedec_2024_rt_amd import scenes

    w = _World(oracle, scenes.make_quad_room(), EYE, AT)
    assert int(w.shaded.sum()) == 2329
    return w


@pytest.mark.parametrize("D", [2, 3, 6])
def test_camera_start_is_the_oracle_s_tail(room, D):
    """path_trace(8, 1) + tail(D - 1) against path_trace(8, D), per channel. Both sides add the same at most D + 1 non-negative binary32
    terms (emission or the depth-0 next-event term, then one term per later depth), only grouped differently: ((t0 + t1) + t2) + ...
    against t0 + ((t1 + t2) + ...). Each of the at most D additions of either side rounds by at most 2^-24 of a partial sum that the
    total bounds, so the two differ by at most 2 D 2^-24 (1 + small) of the total: within (D + 1) 2^-23."""
    for frame in (1, 7, 1000):
        first, full = room.nee(frame, 1), room.nee(frame, D)
        tail, st = room.tail(frame, D - 1, ir.CAMERA)
        assert st["paths"] == int(room.shaded.sum())
        assert (tail >= 0).all() and not tail[~room.shaded].any()
        lit = int((tail > 0).any(axis=1).sum())
        print(f"D = {D} frame {frame}: tail > 0 at {lit} pixels, energy {tail.sum():.4f} of {full.sum():.4f}")
        assert lit >= 300, "the comparison could not fail"
        got = first + tail
        bound = np.float64(D + 1) * 2.0 ** -23 * np.maximum(full, got).astype(np.float64)
        err = np.abs(got.astype(np.float64) - full.astype(np.float64))
        assert (err <= bound).all(), f"D = {D} frame {frame}: {int((err > bound).sum())} channels beyond the bound, max {err.max():.3e}"
        # and it is the tail that closes the gap
        assert (np.abs(first.astype(np.float64) - full) > bound).any()


def test_stats_count_paths_and_rays(room):
    """every started path enters bounce 1; a bounce is one closest-hit ray and, on a shaded hit, one shadow ray"""
    _, s1 = room.tail(7, 1)
    _, s5 = room.tail(7, 5)
    assert s1["paths"] == s1["alive_last"] == s5["paths"] == int(room.shaded.sum())
    assert s1["paths"] <= s1["rays"] <= 2 * s1["paths"] and s1["rays"] < s5["rays"] <= 10 * s5["paths"]
    assert 0 < s5["alive_last"] < s5["paths"]


# measured on this scene and view (bounces 5): over frames 1-40 one path of 40 x 2 329 differs by more than 1e-4 relative between the
# two starts (frame 10; 95 of 2 329 differ in some bit): the surface point from the barycentrics and the one from ro + t rd differ in
# their last bits, and a bounce ray that grazes an edge then lands on the other side. The test runs frames 1-12: 1 of 27 948.
# Cap = 4 x the measured share, and never more than 2 % of the shaded pixels.
GBUFFER_VS_CAMERA_MEASURED = 1


def test_gbuffer_start_against_camera_start(room):
    n = differ = 0
    for frame in range(1, 13):
        g, sg = room.tail(frame, 5, ir.GBUFFER)
        c, sc = room.tail(frame, 5, ir.CAMERA)
        assert sg["paths"] == sc["paths"] == int(room.shaded.sum())
        rel = np.abs(g.astype(np.float64) - c) > 1e-4 * np.maximum(np.abs(g), np.abs(c))
        differ += int(rel.any(axis=1).sum())
        n += sg["paths"]
    print(f"GBUFFER against CAMERA: {differ} of {n} paths differ by more than 1e-4 relative")
    cap = min(4 * GBUFFER_VS_CAMERA_MEASURED, int(0.02 * n))
    assert differ <= cap, (differ, cap)


def test_unbiased_against_the_oracle_s_tail(room):
    """mean over 500 frames of the GBUFFER tail (bounces 5) against the mean of oracle path_trace(8, 6) - path_trace(8, 1) over 500
    frames numbered apart; r15's statistic, bounds and harness"""
    n_px, frames = int(room.shaded.sum()), 500
    ours, truth = _Seq(n_px), _Seq(n_px)
    for f in range(frames):
        ours.add(room.tail(1 + f, 5)[0][room.shaded].sum(axis=1))
        fr = 100001 + f
        truth.add((room.nee(fr, 6).astype(np.float64) - room.nee(fr, 1))[room.shaded].sum(axis=1))
    ours.done(), truth.done()
    d, z = _compare(ours, truth)
    print(f"tail: ours {ours.stat.mean():.6f}  oracle {truth.stat.mean():.6f}  ({d:+.2f} SE, {int((np.abs(z) > 4).sum())} pixels beyond |z| = 4, max {np.abs(z).max():.2f})")
    assert truth.stat.mean() > 0.01
    assert abs(d) <= 4.0
    assert int((np.abs(z) > 4).sum()) <= 6


def test_edges(oracle, room):
    # bounces = 0 writes nothing
    acc = np.full((W * H, 4), 0.25, np.float32)
    st = ir.add(acc, W, H, 3, room.tris, room.vis, room.eye, room.rg, 0)
    assert st == dict(paths=0, rays=0, alive_last=0) and (acc == 0.25).all()
    # an emissive pixel and a sky pixel keep their bytes; .w is unchanged, accumulate 0 and 1 over three frames
    assert room.emissive.any() and room.shaded.any()
    for accumulate in (0, 1):
        opt = oracle.default_options(accumulate=accumulate, max_depth=1)
        acc = np.zeros((W * H, 4), np.float32)
        for frame in (1, 2, 3):
            room.scene.path_trace(8, W, H, frame, room.rg, opt, acc)
            before = acc.copy()
            st = ir.add(acc, W, H, frame, room.tris, room.vis, room.eye, room.rg, 4)
            assert st["paths"] == int(room.shaded.sum())
            assert np.array_equal(_bits(acc[:, 3]), _bits(before[:, 3]))
            assert (acc[:, 3] == (frame if accumulate else 1)).all()
            assert np.array_equal(_bits(acc[~room.shaded]), _bits(before[~room.shaded]))
            assert (acc[room.shaded, :3] > before[room.shaded, :3]).any()


def test_open_sky_ends_paths_without_a_contribution(oracle):
    """make_ledge is open to the sky: a path that leaves adds nothing (08_nee has no sky light), and sky pixels start none"""
    w = _World(oracle, make_ledge(oracle.TRIANGLE), LEDGE_EYE, LEDGE_AT)
    assert w.sky.any() and w.shaded.any()
    t1, s1 = w.tail(3, 1)
    t6, s6 = w.tail(3, 6)
    assert s1["paths"] == s6["paths"] == int(w.shaded.sum())
    assert not t6[~w.shaded].any()
    # a bounce has at most one closest-hit and one shadow ray; paths die on the sky, so far fewer than the closed-room count
    assert s6["alive_last"] < s1["alive_last"] // 4 and s6["rays"] < 2 * 6 * s6["paths"] // 3
    # against the oracle, as in (1)
    full, first = w.nee(3, 7), w.nee(3, 1)
    tail, _ = w.tail(3, 6, ir.CAMERA)
    err = np.abs((first + tail).astype(np.float64) - full)
    assert (err <= 8 * 2.0 ** -23 * np.maximum(full, first + tail)).all()
