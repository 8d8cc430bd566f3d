"""ReSTIR options past the reference's defaults: the HIP path against the oracle, bit for bit, on the option sets of
tests/option_space_cases.py (tests/test_option_space_cpu.py shows on the oracle alone that none of them is trivial).

The library branches on exactly these bounds - more than 3 spatial passes (the windowed halo mark, rt_timing's events, the roles'
ping-pong), a reach above 87 rows (the mark, the strips' halo), more than 5 and more than 8 neighbours (the batched forms, the mark's
quick reject), candidate counts that are no multiple of 8 (09_ris's batches), M near 2^30 (the 64-B record) - and every fallback
behind them is silent when wrong: a missing mark makes a strip gather a stale record, nothing faults.
"""
import math

import numpy as np
import pytest

import option_space_cases as osc
from test_gpu_parity import FOVY, _eq_bits, _res_fields_equal, _setup
from test_mg_native import _Rig

pytestmark = pytest.mark.gpu

RT_ERR_UNSUPPORTED = 5  # include/restir_rt.h


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def tris():
    from cedec_2024_rt_amd import scenes

    return scenes.make_quad_room()


def _shaded(sc, vis):
    return (vis["index"] >= 0) & ~np.isin(vis["index"], sc.lights)


# ------------------------------------------------------------------------------------------ whole frame
@pytest.mark.parametrize("name", osc.names())
def test_frame_equals_oracle(api, oracle, tris, name):
    """rt_frame with default tuning == the oracle's frame, 3 frames: accumulation, pixels, the temporal history handed on, the
    reference's ray count; the frame ends in RT_RES_1 iff the pass count is odd. Which branch each case takes:
    option_space_cases.CASES[name][4]."""
    _, W, H, optkw, _ = osc.CASES[name]
    r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
    st = oracle.new_state(W, H)
    passes = int(opt["spatial_resampling_passes"][0])
    for frame in osc.FRAMES:
        final = r.frame(frame)
        cnt = oracle.new_counters()
        sc.frame(W, H, frame, rg, eyev, opt, st, cnt)
        acc = r.download(api.RT_BUF_ACCUMULATION)
        ref = st["accum"].reshape(acc.shape)
        assert _eq_bits(acc, ref), f"{name} frame {frame}: {int((acc.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum())} pixels differ"
        assert np.array_equal(r.download(api.RT_BUF_PIXELS).reshape(H, W, 4), st["pixels"]), f"{name} frame {frame}: pixels"
        shaded = _shaded(sc, st["vis"])
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_TEMPORAL), st["temporal"], mask=shaded)
        assert not bad, f"{name} frame {frame}: temporal history {bad}"
        assert r.ray_count() == (int(cnt["rays"][0]), int(shaded.sum())), f"{name} frame {frame}: ray count"
        assert final == (api.RT_RES_1 if passes % 2 == 1 else api.RT_RES_0)
    r.close()


# ------------------------------------------------------------------------------------------ kernel by kernel
@pytest.mark.parametrize("name", osc.names(osc.KERNEL_SEQUENCE_GROUPS))
def test_kernel_sequence_equals_oracle(api, oracle, tris, name):
    """the reference's launch sequence, one entry point per kernel: candidates, temporal reuse and the output buffer of EVERY spatial
    pass (pass index 3 and above included: the ping-pong goes on as src/dst swap) against the oracle's, then resolve"""
    _, W, H, optkw, _ = osc.CASES[name]
    r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
    st = oracle.new_state(W, H)
    passes = int(opt["spatial_resampling_passes"][0])
    for frame in osc.FRAMES:
        r.raycast()
        sc.raycast(W, H, rg, st["vis"])
        shaded = _shaded(sc, st["vis"])
        r.generate_candidate(frame, api.RT_RES_0)
        sc.generate_candidate(W, H, frame, st["vis"], eyev, opt, st["r0"])
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_0), st["r0"])
        assert not bad, f"{name} frame {frame}: generate_candidate {bad}"
        r.temporal_resampling(frame, api.RT_RES_TEMPORAL, api.RT_RES_0)
        sc.temporal_resampling(W, H, frame, st["vis"], eyev, opt, st["temporal"], st["r0"])
        bad = _res_fields_equal(r.download(api.RT_BUF_RES_0), st["r0"])
        assert not bad, f"{name} frame {frame}: temporal_resampling {bad}"
        r.save_temporal_reservoir(api.RT_RES_0, api.RT_RES_TEMPORAL)
        oracle.save_temporal_reservoir(W, H, st["r0"], st["temporal"])
        src, dst = api.RT_RES_0, api.RT_RES_1
        osrc, odst = st["r0"], st["r1"]
        for k in range(passes):
            if k:
                src, dst = dst, src
                osrc, odst = odst, osrc
            r.spatial_resampling(frame, k, src, dst)
            sc.spatial_resampling(W, H, frame, k, st["vis"], eyev, opt, osrc, odst)
            bad = _res_fields_equal(r.download(api.RT_BUF_RES_0 + dst), odst, mask=shaded)
            assert not bad, f"{name} frame {frame}: spatial pass {k}: {bad}"
        r.resolve(dst)
        sc.resolve(st["accum"], W, H, st["vis"], eyev, opt, odst)
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"{name} frame {frame}: resolve"
    r.close()


@pytest.mark.parametrize("name,pass_indices", [("passes5", (0, 3, 4)), ("neighbours9", (0, 1, 2))])
def test_spatial_bytes_past_three_passes_and_eight_neighbours(api, oracle, tris, name, pass_indices):
    """rt_spatial_bytes replays a pass's RNG per neighbour: for pass indices 3 and 4 and for 9 neighbours it keeps the invariants
    tests/test_gpu_parity.py::test_full_size_properties_1080p asserts for 3 passes of 5 (bounded by 16 + 152 + N x 92 bytes per shaded
    pixel, the same for every input buffer that shares the G-buffer), splits into 16 per accepted and 76 per merged neighbour, and
    equals the count the oracle's own pass makes (restir_oracle.c o_spatial_resampling)."""
    _, W, H, optkw, _ = osc.CASES[name]
    r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
    st = oracle.new_state(W, H)
    n_nb = int(opt["spatial_resampling_sample_count"][0])
    for frame in (1, 2):
        r.frame(frame)
        sc.frame(W, H, frame, rg, eyev, opt, st)
    shaded = int(_shaded(sc, st["vis"]).sum())
    for k in pass_indices:
        nbytes, accepted = r.spatial_bytes(2, k, api.RT_RES_0)
        assert 16 * W * H + 152 * shaded < nbytes <= 16 * W * H + (152 + n_nb * 92) * shaded, (name, k, nbytes)
        assert (nbytes, accepted) == r.spatial_bytes(2, k, api.RT_RES_1)
        merged, rest = divmod(nbytes - 16 * W * H - 152 * shaded - 16 * accepted, 76)
        assert rest == 0 and 0 < merged <= accepted <= n_nb * shaded, (name, k, nbytes, accepted)
        cnt = oracle.new_counters()
        sc.spatial_resampling(W, H, 2, k, st["vis"], eyev, opt, st["r0"], st["r1"].copy(), cnt=cnt)
        assert (nbytes, accepted, merged) == (int(cnt["spatial_bytes"][0]), int(cnt["spatial_accepted"][0]), int(cnt["spatial_merged"][0])), (name, k)
    r.close()


def test_timing_with_five_passes(api, oracle, tris):
    """rt_timing has events for passes 0..2 only (restir_rt.hip stage_run: `if (k < 3) mark(4 + k)`): with five passes the timed frame
    still computes the untimed frame's bits, every one of the nine figures is finite and non-negative, and the whole frame took time"""
    _, W, H, optkw, _ = osc.CASES["passes5"]
    plain, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
    timed, _, _, _, _ = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
    timed.timing_enable(True)
    for frame in osc.FRAMES:
        plain.frame(frame)
        timed.frame(frame)
        ms = np.float32(list(timed.timing().values()))
        assert len(ms) == 9 and np.isfinite(ms).all() and (ms >= 0).all(), ms
        assert ms[8] > 0, ms
        for buf in (api.RT_BUF_ACCUMULATION, api.RT_BUF_PIXELS, api.RT_BUF_RES_TEMPORAL, api.RT_BUF_RES_0, api.RT_BUF_RES_1):
            assert _eq_bits(plain.download(buf), timed.download(buf)), f"frame {frame}: buffer {buf}"
    plain.close()
    timed.close()


# ------------------------------------------------------------------------------------------ path tracers
@pytest.mark.parametrize("example,optkw", [
    (9, dict(use_shadowed_target_function=1, ris_sample_count=0)),   # no batch at all: the reference still walks two rays to Reservoir{}'s zero position
    (9, dict(use_shadowed_target_function=1, ris_sample_count=7)),   # one partial batch
    (9, dict(use_shadowed_target_function=1, ris_sample_count=9)),   # a partial batch of 1 behind a full one
    (9, dict(use_shadowed_target_function=1, ris_sample_count=17)),  # ... behind two
    (9, dict(use_shadowed_target_function=1, ris_sample_count=33)),  # ... behind four
    (9, dict(ris_sample_count=33)),                                  # the unshadowed loop, one candidate at a time
    (7, dict(max_depth=1)),
    (7, dict(max_depth=12)),
    (8, dict(max_depth=1)),
    (8, dict(max_depth=12)),
])
def test_path_tracers_candidate_batches_and_depths(api, oracle, tris, example, optkw):
    """09_ris with the shadowed target takes its candidates eight at a time (frame_kernels.h pt_bounce): candidate counts that leave a
    partial batch after full ones, and none; 07_pt / 08_nee at one bounce and at twice the default depth. Both forms of rt_tuning key 6
    (one launch per frame, one launch per bounce), two frames each, accumulating: radiance and the reference's ray count."""
    from cedec_2024_rt_amd.types import default_options

    W, H = 64, 36
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    sc = oracle.Scene(tris, use_bvh=True)
    rg = oracle.raygen_lookat(osc.EYE, osc.LOOKAT, (0, 1, 0), FOVY, W, H)
    opt = oracle.default_options(accumulate=1, **optkw)
    want, rays = np.zeros((W * H, 4), np.float32), []
    for frame in (1, 2):
        cnt = oracle.new_counters()
        sc.path_trace(example, W, H, frame, rg, opt, want, cnt=cnt)
        rays.append((want.copy(), int(cnt["rays"][0])))
    assert np.isfinite(want).all() and want[:, :3].max() > 0
    for wavefront in (0, 1):
        r = api.Renderer(W, H)
        r.set_scene(tris)
        r.lookat(osc.EYE, osc.LOOKAT)
        r.set_options(default_options(accumulate=1, **optkw))
        r.tuning(api.Tune.PT_WAVEFRONT, wavefront)
        r.clear()
        for frame in (1, 2):
            r.path_trace(example, frame)
            got = r.download(api.RT_BUF_ACCUMULATION)
            ref, n = rays[frame - 1]
            assert _eq_bits(got, ref), f"example {example} {optkw} wavefront={wavefront} frame {frame}: {int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum())} pixels differ"
            assert r.path_trace_rays() == n, f"example {example} {optkw} wavefront={wavefront} frame {frame}: rays"
        r.close()


# ------------------------------------------------------------------------------------------ M near 2^30
def test_spatial_pass_with_m_above_2_to_24(api, oracle, tris):
    """The 64-B record keeps M in 30 bits and the merge works on (float)M: with M far above 2^24 (where a float no longer holds every
    integer) one spatial pass of 5 neighbours and resolve equal the oracle's on the same input. The M of six reservoirs of at most
    178 956 970 sum to less than 2^30. What the record cannot hold is refused by rt_upload, not truncated."""
    W, H = 80, 45
    r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT)
    assert int(opt["spatial_resampling_sample_count"][0]) == 5 and 6 * 178956970 < 2 ** 30
    r.raycast()
    vis = sc.raycast(W, H, rg)
    shaded = _shaded(sc, vis)
    cand = sc.generate_candidate(W, H, 1, vis, eyev, opt)
    rng = np.random.default_rng(30)
    cand["M"][shaded] = rng.integers(2 ** 24, 178956970, size=int(shaded.sum()), endpoint=True)
    cand["M"][np.flatnonzero(shaded)[:2]] = (2 ** 24, 178956970)
    r.upload(api.RT_BUF_RES_0, cand)
    r.spatial_resampling(1, 0, api.RT_RES_0, api.RT_RES_1)
    want = sc.spatial_resampling(W, H, 1, 0, vis, eyev, opt, cand)
    got = r.download(api.RT_BUF_RES_1)
    bad = _res_fields_equal(got, want, mask=shaded)
    assert not bad, bad
    assert want["M"][shaded].max() > 4 * 2 ** 24 and want["M"].max() < 2 ** 30  # the pass did merge
    r.resolve(api.RT_RES_1)
    acc = np.zeros((W * H, 4), np.float32)
    sc.resolve(acc, W, H, vis, eyev, opt, want)
    assert _eq_bits(r.download(api.RT_BUF_ACCUMULATION), acc)
    cand["M"][np.flatnonzero(shaded)[5]] = 2 ** 30 - 1  # the largest M the record holds goes through ...
    r.upload(api.RT_BUF_RES_0, cand)
    assert np.array_equal(r.download(api.RT_BUF_RES_0)["M"], cand["M"])
    cand["M"][np.flatnonzero(shaded)[5]] = 2 ** 30      # ... one more does not
    with pytest.raises(api.RtError, match=rf"error {RT_ERR_UNSUPPORTED}: .*2\^30"):
        r.upload(api.RT_BUF_RES_0, cand)
    r.close()


def test_options_whose_m_could_reach_2_to_30_are_refused(api, oracle, tris):
    """rt_options_set bounds M by 21 x ris x (1 + neighbours)^passes and refuses what could reach 2^30 (RT_ERR_UNSUPPORTED, the text
    names the bound); negative counts are refused too. A refused set leaves the previous one in place, and the next frame is the
    oracle's under it."""
    from cedec_2024_rt_amd.types import bench_options

    W, H = 80, 45
    kept = dict(spatial_resampling_passes=4, ris_sample_count=9)
    r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **kept)
    before = r.options().tobytes()
    assert before == bench_options(**kept).tobytes()
    for ok, refused in ((dict(ris_sample_count=32, spatial_resampling_sample_count=5, spatial_resampling_passes=7),
                         dict(ris_sample_count=32, spatial_resampling_sample_count=5, spatial_resampling_passes=8)),
                        (dict(ris_sample_count=1, spatial_resampling_sample_count=1, spatial_resampling_passes=25),
                         dict(ris_sample_count=1, spatial_resampling_sample_count=1, spatial_resampling_passes=26))):
        r.set_options(bench_options(**ok))
        assert r.options().tobytes() == bench_options(**ok).tobytes()
        r.set_options(bench_options(**kept))
        with pytest.raises(api.RtError, match=rf"error {RT_ERR_UNSUPPORTED}: .*2\^30"):
            r.set_options(bench_options(**refused))
        assert r.options().tobytes() == before
    for negative in (dict(ris_sample_count=-1), dict(spatial_resampling_sample_count=-1), dict(spatial_resampling_passes=-1)):
        with pytest.raises(api.RtError, match="negative"):
            r.set_options(bench_options(**negative))
        assert r.options().tobytes() == before
    st = oracle.new_state(W, H)
    for frame in (1, 2):
        assert r.frame(frame) == api.RT_RES_0
        sc.frame(W, H, frame, rg, eyev, opt, st)
        acc = r.download(api.RT_BUF_ACCUMULATION)
        assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"frame {frame} after the refusals"
    r.close()


# ------------------------------------------------------------------------------------------ strips, Python driver
STRIP_CASES = {
    # name: (W, H, strips, optkw, reach rows the marks are counted beyond: None = default radius)
    "r60_p4_64x360": (64, 360, 2, dict(spatial_resampling_radius=60.0, spatial_resampling_passes=4), 87),
    "r90_p3_40x540": (40, 540, 2, dict(spatial_resampling_radius=90.0), 87),
    "r90_p3_64x540": (64, 540, 2, dict(spatial_resampling_radius=90.0), 87),
    "p5_96x300": (96, 300, 3, dict(spatial_resampling_passes=5), None),
    "p5_100x300": (100, 300, 3, dict(spatial_resampling_passes=5), None),
    "n9_96x300": (96, 300, 3, dict(spatial_resampling_sample_count=9), None),
}
_strip_refs = {}


def _strip_reference(api, oracle, tris, case):
    """per case, once: the single context's accumulation and pixels of frames 1 and 2, themselves == the oracle's"""
    if case not in _strip_refs:
        W, H, _, optkw, _ = STRIP_CASES[case]
        r, sc, rg, opt, eyev = _setup(api, oracle, tris, W, H, osc.EYE, osc.LOOKAT, **optkw)
        st = oracle.new_state(W, H)
        out = []
        for frame in (1, 2):
            r.frame(frame)
            sc.frame(W, H, frame, rg, eyev, opt, st)
            acc = r.download(api.RT_BUF_ACCUMULATION)
            assert _eq_bits(acc, st["accum"].reshape(acc.shape)), f"{case}: single context against the oracle, frame {frame}"
            assert np.isfinite(acc).all() and _shaded(sc, st["vis"]).mean() > 0.5
            out.append((acc.reshape(H, W, 4).copy(), r.download(api.RT_BUF_PIXELS).reshape(H, W, 4).copy(), r.ray_count()[0]))
        r.close()
        for a in out:
            a[0].setflags(write=False)
            a[1].setflags(write=False)
        _strip_refs[case] = out
    return _strip_refs[case]


def _strip_contexts(api, tris, case):
    from cedec_2024_rt_amd import strips
    from cedec_2024_rt_amd.types import bench_options

    W, H, n, optkw, _ = STRIP_CASES[case]
    opt = bench_options(**optkw)
    halo = math.ceil(strips.halo_bound(float(opt["spatial_resampling_radius"][0])))
    bounds = strips.partition_rows(H, n, halo=halo)
    ctxs = []
    for b in bounds:
        c = api.Renderer(W, H, rows=b, halo=halo)
        c.set_scene(tris)
        c.lookat(osc.EYE, osc.LOOKAT)
        c.set_options(opt)
        ctxs.append(c)
    return ctxs, bounds, halo, int(opt["spatial_resampling_passes"][0])


def _run_strips(api, oracle, tris, case, sparse, tuning=()):
    import torch

    from cedec_2024_rt_amd import strips

    W, H, n, _, _ = STRIP_CASES[case]
    ref = _strip_reference(api, oracle, tris, case)
    ctxs, bounds, halo, _ = _strip_contexts(api, tris, case)
    assert halo == {"r60": 173, "r90": 260}.get(case[:3], 87)
    for c in ctxs:
        for key, value in tuning:
            c.tuning(key, value)
    for frame in (1, 2):
        strips.run_frame_local(ctxs, bounds, frame, torch.device("cuda:0"), halo=halo, sparse=sparse)
        acc_ref, px_ref, rays_ref = ref[frame - 1]
        for c, (a, b) in zip(ctxs, bounds):
            acc = c.download(api.RT_BUF_ACCUMULATION).reshape(c.local_rows, W, 4)[a - c.local_row0: b - c.local_row0]
            assert _eq_bits(acc, acc_ref[a:b]), f"{case} sparse={sparse} frame {frame}: rows {a}:{b}: {int((acc != acc_ref[a:b]).any(axis=2).sum())} pixels differ"
            px = c.download(api.RT_BUF_PIXELS).reshape(c.local_rows, W, 4)[a - c.local_row0: b - c.local_row0]
            assert np.array_equal(px, px_ref[a:b]), f"{case} sparse={sparse} frame {frame}: pixels of rows {a}:{b}"
        assert sum(c.ray_count()[0] for c in ctxs) == rays_ref
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("case", list(STRIP_CASES))
def test_strips_past_the_default_options(api, oracle, tris, case, sparse):
    """Strip contexts driven by strips.run_frame_local with the halo their radius needs (173 rows for radius 60, 260 for radius 90: more
    than SPL_HALO, so rt_halo_mark takes k_halo_mark<false>, as it does for 4 and 5 passes per launch; 9 neighbours take the mark's
    full replay) == the single context, which == the oracle; dense halos and sparse ones, 2 frames."""
    _run_strips(api, oracle, tris, case, sparse)


@pytest.mark.parametrize("case", ["p5_96x300", "r60_p4_64x360"])
def test_strips_with_one_mark_workgroup_per_pass(api, oracle, tris, case):
    """rt_tuning key 26 = 1: k_halo_mark<false> with gridDim.y = 5 and 4, more (tile, pass) workgroups than the windowed form's three
    bitmap slots; sparse halos, same frames"""
    _run_strips(api, oracle, tris, case, True, tuning=((api.Tune.MARK_SPLIT, 1),))


@pytest.mark.parametrize("case", [c for c, v in STRIP_CASES.items() if v[4] is not None])
def test_wide_halos_are_reached_beyond_87_rows(api, tris, case):
    """What makes the wide-radius strip cases above tests of the wide halo: frame 1's need-bitmaps (rt_halo_mark, all passes) hold marks
    in region rows MORE than 87 rows from the strip boundary, on both sides of it. By the Gaussian tail (sigma = radius / 1.96) a few
    hundred are expected per side at radius 90 and about 15 at radius 60; the counts are printed (docs/MEASUREMENT_LOG_r20.md)."""
    import torch

    W, H, n, _, beyond = STRIP_CASES[case]
    ctxs, bounds, halo, passes = _strip_contexts(api, tris, case)
    assert n == 2
    for c in ctxs:
        c.raycast()
    edge = bounds[0][1]
    flags = torch.zeros(halo * W, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for src, dst, row0 in ((ctxs[1], ctxs[0], edge), (ctxs[0], ctxs[1], edge - halo)):
        src.halo_flags_pack(row0, halo, flags.data_ptr())
        src.sync()
        dst.halo_flags_unpack(row0, halo, flags.data_ptr())
        dst.sync()
    counts = {}
    for c, side in ((ctxs[0], 1), (ctxs[1], 0)):
        words = c.halo_bitmap_words(halo)
        nw = (words - 1) // 2
        bm = torch.zeros(passes * words, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.halo_mark(1, 0, passes, side, bm.data_ptr())
        c.sync()
        h = bm.cpu().numpy().view(np.uint32).reshape(passes, words)
        far = total = 0
        for k in range(passes):
            bits = np.unpackbits(h[k, 1:1 + nw].view(np.uint8), bitorder="little")[: halo * W].reshape(halo, W)
            assert int(bits.sum()) == int(h[k, 0])  # word 0: the count the scan left
            # region row i is i + 1 rows from the strip above the boundary (side 1), halo - i rows from the one below it (side 0)
            dist = np.arange(halo) + 1 if side == 1 else halo - np.arange(halo)
            far += int(bits[dist > beyond].sum())
            total += int(bits.sum())
        counts[side] = (far, total)
        print(f"{case}: side {side}: {far} of {total} marks of frame 1 ({passes} passes) lie more than {beyond} rows from the boundary")
    assert counts[0][0] > 0 and counts[1][0] > 0, counts
    for c in ctxs:
        c.close()


def test_halo_of_87_rows_is_too_small_for_radius_31(api, tris):
    """halo_rows_needed grows with the radius: radius 31 needs ceil(31 / 1.96 * 5.6471) = 90 rows, so a strip created with the default
    87 refuses its spatial pass ("too small", and says what it needs) where one created with 90 runs it"""
    from cedec_2024_rt_amd.types import bench_options

    for halo, enough in ((87, False), (89, False), (90, True)):
        c = api.Renderer(32, 200, rows=(0, 100), halo=halo)
        c.set_scene(tris)
        c.lookat(osc.EYE, osc.LOOKAT)
        c.set_options(bench_options(spatial_resampling_radius=31.0))
        c.raycast()
        c.generate_candidate(1)
        if enough:
            c.spatial_resampling(1, 0, api.RT_RES_0, api.RT_RES_1)
        else:
            with pytest.raises(api.RtError, match=rf"halo of {halo} rows is too small: .* needs 90"):
                c.spatial_resampling(1, 0, api.RT_RES_0, api.RT_RES_1)
            c.frame_stage(2, 0)  # the staged frame, which is what a strip runs, refuses at the same place
            with pytest.raises(api.RtError, match="too small"):
                c.frame_stage(2, 1)
        c.close()


# ------------------------------------------------------------------------------------------ strips, native driver
@pytest.mark.parametrize("W,H,halo,optkw", [
    (96, 240, 87, dict(spatial_resampling_passes=4)),                                     # rt_halo_mark_sides with n_pass = 4: k_halo_mark<false>
    (96, 240, 87, dict(spatial_resampling_passes=8, spatial_resampling_sample_count=2)),  # all of the arenas' max_passes = 8 bitmaps per side
    (64, 360, 173, dict(spatial_resampling_radius=60.0)),                                 # rt_mg_create takes the context's halo: 173-row bands
])
def test_native_strips_past_the_default_options(api, tris, W, H, halo, optkw):
    """rt_mg over the LOCAL hub, 2 strips: frames 1..4 (cold, then warm frames whose plan rode on the previous frame's exchange) ==
    the single context: accumulation, pixels, temporal history, rays"""
    bounds = [(0, H // 2), (H // 2, H)]
    rig = _Rig(api, tris, W, H, 2, osc.EYE, osc.LOOKAT, optkw, 0, bounds=bounds, halo=halo)
    for frame in (1, 2, 3, 4):
        rig.frame(frame)
        rig.check(f"{optkw} frame {frame}")
        rig.check_history(f"{optkw} frame {frame}")
    st = rig.mgs[0].stats()
    assert st["frames"] == 4 and st["cold_frames"] == 1 and st["records_sent"] > 0, st
    assert sum(c.ray_count()[0] for c in rig.ctxs) == rig.full.ray_count()[0]
    rig.close()


def test_native_strips_refuse_nine_passes(api, tris):
    """rt_mg's arenas hold 8 passes' bitmaps: 9 passes (an option set rt_options_set accepts) are refused by rt_mg_frame with
    RT_ERR_UNSUPPORTED before anything is enqueued, and the same rt_mg then runs 3-pass frames that equal the single context"""
    from cedec_2024_rt_amd.types import bench_options

    W, H = 96, 240
    nine = dict(spatial_resampling_passes=9, ris_sample_count=1, spatial_resampling_sample_count=1)
    rig = _Rig(api, tris, W, H, 2, osc.EYE, osc.LOOKAT, nine, 0, bounds=[(0, 120), (120, 240)])
    for m in rig.mgs:
        with pytest.raises(api.RtError, match=rf"error {RT_ERR_UNSUPPORTED}: more than 8 spatial passes"):
            m.frame(1)
    assert rig.mgs[0].stats()["frames"] == 0
    for r in rig.everyone():
        r.set_options(bench_options())
    for frame in (1, 2, 3):
        rig.frame(frame)
        rig.check(f"frame {frame} after the refusal")
        rig.check_history(f"frame {frame} after the refusal")
    rig.close()
