"""The plans of tests/stream_delay.py, without a GPU: deterministic per seed, and over the plans every stream is held in every gap
of every script at least once (the second lane wherever the API lets a caller hold it)."""
import stream_delay as sd


def test_scripts_are_the_ones_the_gpu_test_runs():
    scripts = sd.all_scripts()
    names = [s.name for s in scripts]
    assert len(set(names)) == len(names)
    assert len(sd.frame_scripts()) == 15 and len(sd.foreign_scripts()) == len(sd.FOREIGN) == 34
    for s in scripts:
        assert s.steps[-1].op == "checkpoint", f"{s.name}: a script ends with rt_download alone"
        assert all(st.op in sd.OPS for st in s.steps), s.name
    for s in sd.frame_scripts() + [sd.staged_script()]:
        assert s.oracle_frames == sd.FRAMES == 12
    for s in sd.frame_scripts():
        assert [st.args[0] for st in s.steps if st.op == "frame"] == list(range(1, 13))
    for s in sd.foreign_scripts():
        ops = [st.op for st in s.steps]
        assert ops == ["frame"] * 3 + ["foreign"] + ["frame"] * 3 + ["foreign"] + ["frame"] * 2 + ["checkpoint"], s.name
    for s in sd.strip_foreign_scripts():
        ops = [st.op for st in s.steps]
        assert ops == ["strip_frame"] * 3 + ["strip_foreign"] + ["strip_frame"] * 3 + ["strip_foreign"] + ["strip_frame"] * 2 + ["checkpoint"], s.name
        assert (s.W, s.H, s.rows, s.halo) == (96, 300, (100, 200), 87)


def test_plans_are_deterministic_per_seed():
    for s in sd.all_scripts():
        for name in sd.PLANS:
            a, b = sd.plan(name, s), sd.plan(name, sd.all_scripts()[[x.name for x in sd.all_scripts()].index(s.name)])
            assert a == b and len(a) == sd.n_gaps(s), (s.name, name)
        assert sd.plan("random_1", s) != sd.plan("random_2", s), s.name
        assert not any(sd.plan("none", s)), s.name


def test_random_plans_hold_subsets_of_every_size():
    sizes = set()
    for s in sd.all_scripts():
        for name in ("random_1", "random_2"):
            sizes |= {len(h) for h in sd.plan(name, s)}
    assert sizes == {0, 1, 2, 3}


def test_every_stream_is_held_in_every_gap_of_every_script():
    for s in sd.all_scripts():
        plans = [sd.plan(name, s) for name in sd.PLANS]
        for g in range(sd.n_gaps(s)):
            held = frozenset().union(*(p[g] for p in plans))
            assert held == frozenset(sd.allowed(s, g)), (s.name, g, held)
            assert {"main", "tail"} <= held
    # the lane cannot be held only between a stage's _begin and its _fork
    st = sd.staged_script()
    closed = [g for g in range(sd.n_gaps(st)) if "lane" not in sd.allowed(st, g)]
    assert closed and all(st.steps[g + 1].op in ("stage_run_part", "stage_fork") and st.steps[g].op in ("stage_begin", "stage_run_part") for g in closed)
    assert all(sd.allowed(s, g) == sd.STREAMS for s in sd.frame_scripts() + sd.foreign_scripts() + sd.strip_foreign_scripts() for g in range(sd.n_gaps(s)))


def test_strip_plans_hold_main_and_tail_of_every_rank_between_all_sweeps():
    for dense in (False, True):
        single, sweeps = sd.strips_script(dense)
        assert (single.W, single.H, single.oracle_frames) == (96, 300, 12) and sd.STRIP_HALO == 87
        plans = [sd.plan(name, sweeps) for name in sd.STRIP_PLANS]
        assert all(len(p) == 64 for p in plans)
        for g in range(64):
            assert frozenset().union(*(p[g] for p in plans)) == {"main", "tail"}
        assert sd.plan("random_1", sweeps) == sd.plan("random_1", sd.strips_script(dense)[1])


def test_alternating_plan_alternates():
    p = sd.plan("main_and_tail_alternating", sd.frame_scripts()[0])
    assert p[:4] == [frozenset({"main"}), frozenset({"tail"}), frozenset({"main"}), frozenset({"tail"})]


def test_delay_is_eight_frames_within_one_and_four_milliseconds():
    assert sd.delay_ns(20e-6) == 1_000_000
    assert sd.delay_ns(250e-6) == 2_000_000
    assert sd.delay_ns(500e-6) == 4_000_000
    assert sd.delay_ns(501e-6) is None  # too large an image for this test: shrink it, the cap stays
    assert sd.NS_MAX < 5_000_000


def test_a_twelve_frame_script_holds_its_streams_for_less_than_three_tenths_of_a_second():
    for s in sd.all_scripts():
        for name in sd.PLANS:
            p = sd.plan(name, s)
            # holds of one stream serialise, holds of different streams overlap
            # (the staged script has a gap per stage call: it fits up to 1.5 ms, the hold of a 96x54 frame of 187 us; the GPU test asserts it)
            ns = 1_500_000 if s.name == "staged_two_lanes" else sd.NS_MAX
            worst = max(sum(w in h for h in p) for w in sd.STREAMS) * ns * 1e-9
            assert worst < 0.3, (s.name, name, worst)
