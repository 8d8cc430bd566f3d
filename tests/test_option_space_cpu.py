"""The oracle alone on every option set of tests/option_space_cases.py: what keeps the GPU comparisons of
tests/test_gpu_option_space.py from being trivial (a device that equals an all-sky, all-empty or never-merging oracle frame has
shown nothing about pass index 3, the 9th neighbour or a reach of 260 rows)."""
import numpy as np
import pytest

import option_space_cases as osc

FOVY = np.float32(np.pi) / np.float32(4)
_tris = None


def oracle_frames(oracle, name):
    """(scene, shaded mask, state after the last frame) of one case: 3 oracle frames, portable math"""
    global _tris
    from cedec_2024_rt_amd import scenes

    if _tris is None:
        _tris = scenes.make_quad_room()
    _, W, H, optkw, _ = osc.CASES[name]
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(_tris, use_bvh=True)
    rg = oracle.raygen_lookat(osc.EYE, osc.LOOKAT, (0, 1, 0), FOVY, W, H)
    st = oracle.new_state(W, H)
    opt = oracle.bench_options(**optkw)
    for frame in osc.FRAMES:
        sc.frame(W, H, frame, rg, np.asarray(osc.EYE, np.float32), opt, st)
    shaded = (st["vis"]["index"] >= 0) & ~np.isin(st["vis"]["index"], sc.lights)
    return sc, shaded, st, opt


def test_every_case_names_its_branch():
    assert len(osc.CASES) == 26
    for name, (group, W, H, optkw, branch) in osc.CASES.items():
        assert group in ("passes", "radius", "radius_tall", "neighbours", "candidates") and len(branch) > 20, name
        assert (W, H) == ((64, 540) if group == "radius_tall" else (80, 45)), name


@pytest.mark.parametrize("name", osc.names())
def test_oracle_frames_are_not_trivial(oracle, name):
    """finite radiance, most pixels shaded, and the spatial passes merged (or provably did not, where no neighbour can differ from
    the pixel itself)"""
    _, shaded, st, opt = oracle_frames(oracle, name)
    passes = int(opt["spatial_resampling_passes"][0])
    assert np.isfinite(st["accum"]).all()
    assert shaded.mean() > 0.5, shaded.mean()
    final = st["r1"] if passes % 2 == 1 else st["r0"]
    m_final, m_temporal = final["M"][shaded].astype(np.int64), st["temporal"]["M"][shaded].astype(np.int64)
    print(f"{name}: shaded {shaded.mean():.3f}, median M {np.median(m_final):.0f} (post-temporal {np.median(m_temporal):.0f}), max M {m_final.max()}")
    assert (m_final >= 0).all() and m_final.max() < 2 ** 30
    if int(opt["ris_sample_count"][0]) == 0:
        assert not st["r0"]["M"].any() and not st["r1"]["M"].any() and not st["temporal"]["M"].any()
    elif name in osc.NO_MERGE:
        assert np.array_equal(m_final, m_temporal)
    elif name in osc.SPARSE_MERGE:
        assert (m_final > m_temporal).sum() >= 100
    else:
        assert np.median(m_final) > np.median(m_temporal)
    assert (m_final >= m_temporal).all()
