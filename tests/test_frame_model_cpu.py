"""tests/frame_model.py without a GPU: anchored to the six private CPU frames of the per-feature GPU test files,
the conditions every case of tests/test_gpu_feature_matrix.py has to meet by the model alone, and the census: the forms the model
predicts over the matrix are the rows of csrc/stage0_forms.h, no more and no fewer."""
import numpy as np
import pytest

import feature_matrix_cases as fc
import frame_model as fm
import light_sampling_ref as ls
import temporal_unbiased_ref as tu
from test_stage0_forms_cpu import walk


@pytest.fixture(scope="module")
def scenes(oracle):
    return fm.Scenes(oracle)


def _same(m, st, last, out, shaded, what):
    """accumulation, pixels, the last pass's records and the history: bit for bit"""
    assert fc.eq_bits(m.accum, st["accum"]), f"{what}: accumulation"
    assert np.array_equal(m.pixels, st["pixels"]), f"{what}: pixels"
    assert not fc.res_diff(m.buf[fm.NAMES[out]], last, shaded), f"{what}: records"
    assert not fc.res_diff(m.buf["temporal"], st["temporal"], shaded), f"{what}: temporal history"


def _model(oracle, scenes, W, H, tris, opt):
    m = fm.FrameModel(oracle, W, H, scenes=scenes)
    m.set_scene(tris)
    m.set_options(opt)
    return m


# ------------------------------------------------------------------------------------------------------------------ anchor
def test_anchor_light_sampling(oracle, scenes):
    """tests/test_gpu_light_sampling.py: power candidates, a camera that stands still"""
    from test_gpu_light_sampling import _Cpu

    W, H = 37, 29
    opt = oracle.bench_options(accumulate=1)
    tris = ls.make_lamp_room()
    world = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=ls.LAMP_EYE, at=ls.LAMP_AT)
    cpu = _Cpu(oracle, world, W, H, opt)
    m = _model(oracle, scenes, W, H, tris, opt)
    m.light_sampling("power")
    m.lookat(ls.LAMP_EYE, ls.LAMP_AT)
    assert fc.eq_bits(m.view.rg, cpu.rg) and np.array_equal(m.view.shaded, cpu.shaded)
    for frame in (1, 2, 3, 4):
        want = m.frame(frame)
        _same(m, cpu.st, cpu.frame(frame), want.out, cpu.shaded, f"frame {frame}")


def test_anchor_temporal_reproject(oracle, scenes):
    """tests/test_gpu_temporal_reproject.py: an orbit, the reprojected merge"""
    from test_gpu_temporal_reproject import ORBIT_STEP, _Cpu
    from test_temporal_reproject_cpu import View, _orbit

    W, H = 37, 29
    opt = oracle.bench_options(accumulate=1)
    tris = ls.make_lamp_room()
    world = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True))
    cpu = _Cpu(oracle, world, W, H, opt)
    m = _model(oracle, scenes, W, H, tris, opt)
    m.temporal_reprojection(True)
    for k in range(4):
        view = View(oracle, world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT_STEP * k))
        m.lookat(view.eye, view.at)
        want = m.frame(1 + k)
        _same(m, cpu.st, cpu.frame(1 + k, view), want.out, view.shaded, f"frame {1 + k}")
    assert m.seen["reprojected_from_another_pixel"] > 0


def test_anchor_temporal_motion(oracle, scenes):
    """tests/test_gpu_temporal_motion.py: the moving box under an orbit, power candidates"""
    from test_gpu_temporal_motion import FRAME_ORBIT, _Cpu, _frame_worlds
    from test_temporal_motion_cpu import BOX_HI, BOX_LO, Worlds
    from test_temporal_reproject_cpu import _orbit

    W, H = 37, 29
    opt = oracle.bench_options()
    worlds = Worlds(oracle)
    ws = _frame_worlds(worlds)
    cpu = _Cpu(oracle, W, H, opt, power=True)
    m = _model(oracle, scenes, W, H, ws[0]["tris"], opt)
    m.temporal_reprojection(True)
    m.temporal_motion(True)
    m.light_sampling("power")
    for k, w in enumerate(ws):
        view = worlds.view(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, FRAME_ORBIT * k))
        if k:
            m.update_scene(w["tris"][BOX_LO:BOX_HI], BOX_LO)
            assert m.motion_range() == dict(lo=BOX_LO, hi=BOX_HI, generation=k - 1)
        m.lookat(view.eye, view.at)
        want = m.frame(1 + k)
        _same(m, cpu.st, cpu.frame(1 + k, w, view), want.out, view.shaded, f"frame {1 + k}")
        assert m.tag["temporal"].gen == k
    assert m.seen["motion_valid"] > 0 and m.seen["motion_elsewhere"] > 0


def test_anchor_temporal_unbiased(oracle, scenes):
    """tests/test_gpu_temporal_unbiased.py: the 1/Z merge over an orbit with the unbiased passes; the counters it sums"""
    from cedec_2024_rt_amd import scenes as product_scenes
    from test_gpu_temporal_unbiased import ORBIT_STEP, ORBIT_STEPS, QUAD_AT, QUAD_EYE, _Cpu
    from test_temporal_reproject_cpu import View, _orbit

    W, H = 37, 29
    opt = oracle.bench_options()
    tris = product_scenes.make_quad_room()
    world = dict(tris=tris, scene=oracle.Scene(tris, use_bvh=True), eye=QUAD_EYE, at=QUAD_AT)
    cpu = _Cpu(oracle, world, W, H, opt, spatial_unbiased=True)
    m = _model(oracle, scenes, W, H, tris, opt)
    m.temporal_reprojection(True)
    m.temporal_unbiased(True)
    m.spatial_unbiased(True)
    m.walk_stats_enable(True)
    for k in range(ORBIT_STEPS + 1):
        view = View(oracle, world, W, H, *_orbit(QUAD_EYE, QUAD_AT, -ORBIT_STEP * (ORBIT_STEPS - k)))
        m.lookat(view.eye, view.at)
        want = m.frame(1 + k)
        _same(m, cpu.st, cpu.frame(1 + k, view), want.out, view.shaded, f"frame {1 + k}")
    assert m.unbiased_stats == cpu.counts and cpu.counts["excluded"] > 0
    assert (m.reproject_stats["merged"], m.reproject_stats["valid"]) == (cpu.counts["merged"], cpu.gathered)


def test_anchor_light_follow(oracle, scenes):
    """tests/test_gpu_light_follow.py: the moving, dimming panel under an orbit with the reprojected merge"""
    from test_gpu_light_follow import FRAMES, ORBIT, STEP, _Cpu, _dim
    from test_light_follow_cpu import BASE, P0, Worlds, move
    from test_temporal_reproject_cpu import _orbit

    W, H = 19, 7
    opt = oracle.bench_options()
    worlds = Worlds(oracle)
    cpu = _Cpu(oracle, W, H, opt, True, True)
    m = _model(oracle, scenes, W, H, BASE, opt)
    m.temporal_reprojection(True)
    m.temporal_light_motion(True)
    t = BASE
    for k in range(FRAMES):
        if k:
            t = _dim(move(t, STEP), k)
            m.update_scene(t[P0:P0 + 2], P0)
            assert m.last_rebased == 4, "the three logical buffers and the look-ahead's"
        w = worlds.of(t)
        view = worlds.view_at(w, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, ORBIT * k))
        m.lookat(view.eye, view.at)
        want = m.frame(1 + k)
        _same(m, cpu.st, cpu.frame(1 + k, w, view), want.out, view.shaded, f"frame {1 + k}")
    assert m.seen["records_moved"] > 0


def test_anchor_light_grid(oracle, scenes):
    """tests/test_gpu_light_grid.py: the grid's candidates with the box followed"""
    from test_gpu_light_grid import _Cpu
    from test_temporal_motion_cpu import BOX_HI, BOX_LO, Worlds, move
    from test_temporal_reproject_cpu import _orbit

    W, H = 37, 29
    opt = oracle.bench_options()
    ws = Worlds(oracle)
    cpu = _Cpu(oracle, W, H, opt, grid=(16, 64))
    t = move(ws.base, (0.0, 0.0, -2.0))
    m = _model(oracle, scenes, W, H, t, opt)
    m.temporal_reprojection(True)
    m.temporal_motion(True)
    m.light_grid(16, 64)
    for k in range(4):
        if k:
            t = move(t, (0.0, 0.0, 1.0))
            m.update_scene(t[BOX_LO:BOX_HI], BOX_LO)
        world = ws.of(t)
        view = ws.view(world, W, H, *_orbit(ls.LAMP_EYE, ls.LAMP_AT, 0.1 * k))
        m.lookat(view.eye, view.at)
        want = m.frame(1 + k)
        _same(m, cpu.st, cpu.frame(1 + k, world, view, temporal="motion"), want.out, view.shaded, f"frame {1 + k}")


# -------------------------------------------------------------------------------------------------- conditions and census
@pytest.fixture(scope="module")
def matrix(oracle, scenes):
    """every case of the matrix through the model alone, once: {case: (launches, model)}"""
    return {c: fc.run(oracle, scenes, c) for c in fc.CASES}


def test_every_case_contains_what_it_names(matrix):
    for c, (_, m) in matrix.items():
        fc.conditions(c, m)


def test_grid_cases_differ_from_the_uniform_ones(oracle, scenes, matrix):
    for c, (_, m) in matrix.items():
        if c.selection == "grid":
            twin = c._replace(selection="uniform")
            u = (matrix[twin] if twin in matrix else fc.run(oracle, scenes, twin))[1]
            assert fc.res_diff(m.buf["temporal"], u.buf["temporal"], m.view.shaded), fc.case_id(c)


def test_census_product(matrix):
    """the union of the predicted forms over the matrix is exactly GEN_FORMS and TEMPORAL_FORMS of the product build, plus the unbiased
    merge: a row added to csrc/stage0_forms.h without a case fails here"""
    seen = set().union(*(l for l, _ in matrix.values()))
    rows = walk(False)["tables"]
    assert len(rows) == 48  # 42 forms of k_generate_candidate, 6 of k_temporal
    assert seen == rows | {"k_temporal_unbiased"}, (sorted(rows - seen), sorted(seen - rows))


def test_census_experiments(oracle, scenes, matrix):
    """with the experiments library's six rows: 48 forms of k_generate_candidate"""
    seen = set().union(*(l for l, _ in matrix.values()))
    for c in fc.EXP_CASES:
        seen |= fc.run(oracle, scenes, c)[0]
    rows = walk(True)["tables"]
    assert len([r for r in rows if r.startswith("k_generate_candidate")]) == 48
    assert seen == rows | {"k_temporal_unbiased"}, (sorted(rows - seen), sorted(seen - rows))


@pytest.mark.parametrize("seed,W,H", fc.SOAK_CASES)
def test_every_soak_seed_contains_what_it_has_to(oracle, scenes, seed, W, H):
    """a reuse frame, a motion launch with a valid history elsewhere, a re-base with records moved, an unbiased launch, a refused call
    and a grid frame right after a light move: at least one each, by the model alone"""
    m = fc.soak(oracle, scenes, seed, W, H)
    assert not [k for k in fc.SOAK_NEEDS if m.seen[k] == 0], m.seen


def test_refusals_by_the_model(oracle, scenes):
    """the refusals the matrix checks on the device, stated once here: codes and texts"""
    m = _model(oracle, scenes, 8, 8, fc.start_scene(), oracle.bench_options())
    m.lookat(*fc.orbit(0.0))
    m.temporal_reprojection(True)
    assert m.temporal_motion(True).code == 0
    r = m.temporal_unbiased(True)
    assert (r.code, r.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_UNBIASED_MOTION) and not m.t_unbiased
    m.temporal_motion(False)
    assert m.temporal_unbiased(True).code == 0
    r = m.temporal_motion(True)
    assert (r.code, r.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_MOTION_UNBIASED) and not m.motion
    assert m.frame(1).code == 0
    m.set_options(oracle.bench_options(use_shadowed_target_function=1))
    assert m.frame(2).code == 0, "the camera stands still: no unbiased launch"
    m.lookat(*fc.orbit(0.1))
    before = {k: v.copy() for k, v in m.buf.items()}
    r = m.frame(3)
    assert (r.code, r.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_UNBIASED_SHADOWED)
    assert all(fc.eq_bits(before[k], m.buf[k]) for k in before)
    m.temporal_unbiased(False)
    m.spatial_unbiased(True)
    r = m.frame(3)
    assert (r.code, r.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_SPATIAL_SHADOWED)
    m.set_options(oracle.bench_options(spatial_resampling_sample_count=6))
    r = m.frame(3)
    assert (r.code, r.error) == (fm.RT_ERR_UNSUPPORTED, fm.E_SPATIAL_COUNT % 6)
    m.spatial_unbiased(False)
    assert m.frame(3).code == 0
    assert tu.UNBIASED == 2
