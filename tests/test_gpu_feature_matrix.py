"""The ReSTIR toggles on the device against tests/frame_model.py, in every combination: every row of GEN_FORMS and
TEMPORAL_FORMS (csrc/stage0_forms.h) in a world where the box, the panel and the camera all move between two frames; the refusals
mid-sequence; and a soak that feeds two contexts (default knobs, every shortcut off) and the model one random order of events.

Every assertion is bit-for-bit equality or an integer count. The cases and the driver are tests/feature_matrix_cases.py;
tests/test_frame_model_cpu.py has shown by the model alone that every case contains what it names."""
import os

import numpy as np
import pytest

import feature_matrix_cases as fc
import frame_model as fm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def scenes(oracle):
    return fm.Scenes(oracle)


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_case_equals_the_model(api, oracle, scenes, c):
    fc.run(oracle, scenes, c, api=api)


@pytest.mark.parametrize("c", fc.EXP_CASES, ids=fc.case_id)
def test_experiment_rows_equal_the_model(api, oracle, scenes, c):
    """rt_tuning 11 and 12 of the experiments library: their six rows run, and in the same sequence the grid and a reprojecting launch
    are refused"""
    if not os.path.exists(api.EXP_LIB_PATH):
        pytest.skip("librestir_rt_exp.so is not built")
    fc.run(oracle, scenes, c, api=api)
    p = fc.Pair(oracle, c.W, c.H, scenes, api=api, exp=True)
    try:
        fc.setup(p, oracle, c, fc.start_scene())
        p.lookat(*fc.orbit(0.0))
        assert p.frame(1).code == 0
        p.light_grid(*fc.GRID)
        want = p.frame(2)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_EXP_GRID)
        p.light_grid(0, 0)
        assert p.frame(2).code == 0
        p.temporal_reprojection(True)
        assert p.frame(3).code == 0, "the camera stands still: no reprojecting launch"
        p.lookat(*fc.orbit(fc.ORBIT))
        want = p.frame(4)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_EXP_REPROJECT)
        p.temporal_reprojection(False)
        assert p.frame(4).code == 0
    finally:
        p.close()


@pytest.mark.parametrize("seed,W,H", fc.SOAK_CASES)
def test_soak_whole_frame_context(api, oracle, scenes, seed, W, H):
    """32 frames under a random order of events (tests/feature_matrix_cases.py: soak): context A with default knobs, context B with
    every shortcut off and the model hold the same bytes and tags after every frame, and A traces primary rays exactly where the model
    says a frame does. rt_walk_stats_enable is off: G-buffer reuse and the look-ahead really happen. Every message carries the events so far"""
    fc.soak(oracle, scenes, seed, W, H, api=api)


def test_a_light_selection_switched_under_a_still_camera_drops_the_look_ahead(api, oracle, scenes):
    """default knobs, rt_walk_stats_enable off, no camera call: a frame would take the look-ahead's candidates, which the frame before
    drew from the tables of the selection before. rt_light_grid (on, other settings, off) and rt_light_sampling between two such
    frames: the next frame holds the model's bytes and traces primary rays where the model says"""
    p = fc.Pair(oracle, 37, 29, scenes, api=api)
    try:
        p.set_scene(fc.start_scene())
        p.set_options(oracle.bench_options(accumulate=1))
        p.lookat(*fc.orbit(0.0))
        n = 0
        for switch in (None, None, lambda: p.light_grid(16, 64), None, lambda: p.light_grid(4, 8), lambda: p.light_grid(0, 0), None,
                       lambda: p.light_sampling("power"), None, lambda: p.light_sampling("uniform"), lambda: p.light_grid(2, 3)):
            if switch:
                switch()
            n += 1
            assert p.frame(n).code == 0
        # a switch counts as an option change: the frame after it traces again, the four others reuse
        assert p.m.seen["reuse_frames"] == 4 and p.r[0].primary_launches() == p.m.primary_launches == n - 4
    finally:
        p.close()


def test_refusals_mid_sequence(api, oracle, scenes):
    """every refusal of the model: the code, the text, nothing changed (Pair checks rt_state_epoch, the three buffers, their tags and the
    moved range around every refused call), and the sequence goes on once the option is withdrawn"""
    W, H = 37, 29
    p = fc.Pair(oracle, W, H, scenes, api=api)
    try:
        t = fc.start_scene()
        p.set_scene(t)
        p.set_options(oracle.bench_options())
        p.tuning(16, 0)
        p.temporal_reprojection(True)
        p.temporal_light_motion(True)
        p.walk_stats_enable(True)
        p.lookat(*fc.orbit(0.0))
        assert p.frame(1).code == 0
        # the two toggles that refuse each other, in either order
        assert p.temporal_motion(True).code == 0
        want = p.temporal_unbiased(True)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_UNBIASED_MOTION)
        t = fc.move(t, fc.BOX_STEP, fc.BOX_LO, fc.BOX_HI - fc.BOX_LO)
        p.update_scene(t, fc.BOX_LO, fc.BOX_HI - fc.BOX_LO, "box")
        p.lookat(*fc.orbit(fc.ORBIT))
        assert p.frame(2).code == 0
        assert p.temporal_motion(False).code == 0 and p.temporal_unbiased(True).code == 0
        want = p.temporal_motion(True)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_MOTION_UNBIASED)
        p.lookat(*fc.orbit(2 * fc.ORBIT))
        assert p.frame(3).code == 0  # an unbiased launch
        # an unbiased launch under the shadowed target function: fine while the camera stands still, refused once it moves
        p.set_options(oracle.bench_options(use_shadowed_target_function=1))
        assert p.frame(4).code == 0
        p.lookat(*fc.orbit(3 * fc.ORBIT))
        want = p.frame(5)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_UNBIASED_SHADOWED)
        p.temporal_unbiased(False)
        assert p.frame(5).code == 0
        # the unbiased passes: the shadowed target function, more than five neighbours
        p.spatial_unbiased(True)
        want = p.frame(6)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_SPATIAL_SHADOWED)
        p.set_options(oracle.bench_options(spatial_resampling_sample_count=6))
        t = fc.move(t, fc.PANEL_STEP, fc.P0, 2)
        p.update_scene(t, fc.P0, 2, "panel")
        want = p.frame(6)
        assert (want.code, want.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_SPATIAL_COUNT % 6)
        p.set_options(oracle.bench_options())
        assert p.frame(6).code == 0
        p.spatial_unbiased(False)
        assert p.frame(7).code == 0
        p.check_stats()
        assert p.m.seen["unbiased_launches"] > 0 and p.m.seen["motion_launches"] > 0 and p.m.seen["records_moved"] > 0
    finally:
        p.close()
