"""tests/bvh_build_scenes.py on the CPU: the scenes are what tests/test_gpu_bvh_build.py takes them for (sizes, coinciding
centroids, forced first splits, a first fragment length far below the walls), and the brute-force reference alone meets the hit
fraction the device tests assert."""
import numpy as np
import pytest

import bvh_build_scenes as S


@pytest.fixture(scope="module")
def portable(oracle):
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    return oracle


def _centroids(v, pad=0.0):
    lo, hi = v.min(axis=1) - np.float32(pad), v.max(axis=1) + np.float32(pad)
    return (np.float32(0.5) * (lo + hi)).astype(np.float32)


@pytest.mark.parametrize("name", S.ALL)
def test_a_fifth_of_the_rays_hit(portable, name):
    v, rays, ref, _ = S.reference(portable, name)
    assert rays.shape == (S.N_RAYS, 8) and rays.dtype == np.float32 and v.dtype == np.float32
    assert np.isfinite(v).all() and np.isfinite(rays[:, :7]).all()
    hit = ref[:, 3].view(np.int32) >= 0
    assert hit.mean() >= S.MIN_HIT_FRACTION
    if name.startswith(("clusters:", "degenerate:e_far")):  # both clusters are hit
        idx = ref[hit, 3].view(np.int32)
        first = int(name.split(":")[1].split("+")[0]) if name.startswith("clusters:") else len(v) // 2
        assert (idx < first).sum() >= 20 and (idx >= first).sum() >= 20


def test_sizes_and_generic_position():
    for name in S.SOUPS + S.LARGE:
        v, _, _ = S.scene(name)
        assert len(v) == int(name.split(":")[1])
        c = _centroids(v)
        for a in range(3):
            assert len(np.unique(c[:, a])) == len(v), f"{name}: two centroids share coordinate {a}"
    assert sorted(len(S.scene(n)[0]) for n in S.SOUPS) == sorted(S.REGIME_SIZES)


@pytest.mark.parametrize("na,nb", S.CLUSTER_SIZES)
def test_cluster_scenes_force_the_first_split(na, nb):
    """on every axis the centroids of the first cluster lie in bin 0 of 32 and those of the second in bin 31, by the builders'
    binary32 expression, with the build's pad or without"""
    v, _, _ = S.scene(f"clusters:{na}+{nb}")
    assert len(v) == na + nb
    for pad in (0.0, 4e-5 * 51):
        c = _centroids(v, pad)
        for a in range(3):
            clo, chi = c[:, a].min(), c[:, a].max()
            b = np.clip(((c[:, a] - clo) * (np.float32(32) / (chi - clo))).astype(np.int32), 0, 31)
            assert (b[:na] == 0).all() and (b[na:] == 31).all()


@pytest.mark.parametrize("n", S.DEGENERATE_SIZES)
def test_degenerate_centroids_coincide_where_they_should(n):
    pad = np.float32(4e-5 * 10)
    for kind, axes in (("a_copies", (0, 1, 2)), ("b_concentric", (0, 1, 2)), ("c_line", (1, 2)), ("d_plane", (1,))):
        v, _ = S.degenerate(kind, n)
        assert len(v) == n
        c = _centroids(v, pad)
        for a in range(3):
            same = len(np.unique(c[:, a])) == 1
            assert same == (a in axes), f"{kind}: axis {a}"
    v, _ = S.degenerate("b_concentric", n)
    ext = (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    assert ext.max() / ext.min() > (100 if n < 100 else 500)
    v, _ = S.degenerate("e_far_clusters", n)
    assert np.abs(v[: n // 2]).max() < 2 and (v[n // 2:, :, 0] > 999990).all()
    v, _ = S.degenerate("f_enclosed", n)
    assert (v[-1].min(axis=0) < v[:-1].reshape(-1, 3).min(axis=0)).all() and (v[-1].max(axis=0) > v[:-1].reshape(-1, 3).max(axis=0)).all()


def test_budget_scene_starts_far_below_its_walls():
    v = S.budget_scene(2000)
    ext = (v.max(axis=1) - v.min(axis=1)).max(axis=1)
    L0 = S.split_length(v, 10.0)
    assert L0 < 0.01 and 150 <= (ext > 1000 * L0).sum() <= 250
