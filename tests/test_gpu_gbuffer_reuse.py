"""rt_gbuffer_reuse: a staged frame traces no primary rays while the G-buffer of the current camera / scene / options is still there.

The primary ray of a pixel is shoot(xi / W, yi / H) (examples/10_restir_di/10_restir_di.cu:17-24): no jitter, no frame number. Every
comparison here is bit for bit, after every frame, on RT_BUF_ACCUMULATION, RT_BUF_PIXELS, RT_BUF_VISIBILITY and every field of
RT_BUF_RES_TEMPORAL but `pad`, against (a) a context with rt_gbuffer_reuse(0) and (b) a context driven by frame_by_kernels (the
reference's launch sequence, which always calls rt_raycast). rt_primary_launches shows which frames traced, without timing anything.

100 x 76 on the bench scene: the width is no multiple of the 8-pixel tile, there are more than eight tile rows (the XCD interleave
wraps) and the last tile row is partial.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 100, 76
FOVY = np.float32(np.pi) / np.float32(4)
EYE2 = (-1.25, 22.6, -6.1)
AT2 = (5.0, 20.5, 1.9)
RADIUS2 = 17.0
N_FRAMES = 16
RT_ERR_UNSUPPORTED = 5  # include/restir_rt.h
CHANGES = (1, 5, 8, 11, 13)  # frames that must trace: the first, and the first after each change of script A


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def api():
    from cedec_2024_rt_amd import api as _api

    return _api


@pytest.fixture(scope="module")
def scenes():
    from cedec_2024_rt_amd import scenes as s

    return s


@pytest.fixture(scope="module")
def world(scenes):
    """the bench scene, and the same with the first half of the light span moved"""
    A = scenes.make_blocks_restir()
    lights = scenes.light_indices(A)
    lo, hi = int(lights.min()), int(lights.max()) + 1
    mid = lo + max(1, (hi - lo) // 2)
    mask = np.zeros(len(A), bool)
    mask[lights[lights < mid]] = True
    assert mask.any()
    B = scenes.move_triangles(A, mask, (0.25, 0.125, -0.5))
    return dict(A=A, B=B, lo=lo, mid=mid, eye=scenes.BLOCKS_RESTIR_EYE, at=scenes.BLOCKS_RESTIR_LOOKAT)


def _renderer(api, world, tune=(), reuse=True, **kw):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H, **kw)
    r.set_scene(world["A"])
    r.lookat(world["eye"], world["at"])
    r.set_options(bench_options())
    for k, v in tune:
        r.tuning(k, v)
    if not reuse:
        r.gbuffer_reuse(False)
    return r


def _snapshot(api, r):
    return dict(acc=r.download(api.RT_BUF_ACCUMULATION), pix=r.download(api.RT_BUF_PIXELS), vis=r.download(api.RT_BUF_VISIBILITY),
                hist=r.download(api.RT_BUF_RES_TEMPORAL))


def _same(a, b, what):
    for k in ("acc", "pix", "vis"):
        assert _eq_bits(a[k], b[k]), f"{what}: {k}: {int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum())} bytes differ"
    for f in a["hist"].dtype.names:
        if f != "pad":
            assert _eq_bits(a["hist"][f], b["hist"][f]), f"{what}: temporal history, field {f}"


def _script_a(api, world, r, step):
    """frames 1-4; lookat, 5-7; rt_scene_update, 8-10; set_options, 11-12; RT_BUF_VISIBILITY down and up again, 13; a bare rt_raycast,
    14; 15-16. Returns per frame the four buffers, rt_primary_launches after it, and the count around the bare rt_raycast."""
    from cedec_2024_rt_amd.types import bench_options

    snaps, counts, bare = [], [], None
    for f in range(1, N_FRAMES + 1):
        if f == 5:
            r.lookat(EYE2, AT2)
        if f == 8:
            r.update_scene(world["B"][world["lo"]:world["mid"]], world["lo"])
        if f == 11:
            r.set_options(bench_options(spatial_resampling_radius=RADIUS2))
        if f == 13:
            r.upload(api.RT_BUF_VISIBILITY, r.download(api.RT_BUF_VISIBILITY))
        if f == 14:
            before = r.primary_launches()
            r.raycast()
            bare = (before, r.primary_launches())
        step(f)
        snaps.append(_snapshot(api, r))
        counts.append(r.primary_launches())
    return snaps, counts, bare


@pytest.fixture(scope="module")
def kernel_sequence(api, world):
    """(b): script A through frame_by_kernels, computed once"""
    r = _renderer(api, world)
    out = _script_a(api, world, r, r.frame_by_kernels)
    r.close()
    return out


_RUNS = {}


def _run_a(api, world, name):
    """script A on a reusing context and on (a) a context with rt_gbuffer_reuse(0), under the same tuning; computed once per form"""
    if name not in _RUNS:
        tune = ((api.Tune.SPEC, 0), (api.Tune.TAIL, 0)) if name == "headline" else ()
        got = {}
        for reuse in (True, False):
            r = _renderer(api, world, tune, reuse=reuse)
            got[reuse] = _script_a(api, world, r, r.frame)
            r.close()
        _RUNS[name] = got
    return _RUNS[name]


@pytest.mark.parametrize("form", ["headline", "look_ahead"])
def test_script_a_reuses_and_matches_tracing_frames_and_the_kernel_sequence(api, world, kernel_sequence, form):
    """`headline`: Tune.SPEC = 0, Tune.TAIL = 0, the frames bench.py's value times; `look_ahead`: the defaults."""
    runs = _run_a(api, world, form)
    snaps, counts, bare = runs[True]
    off_snaps, off_counts, off_bare = runs[False]
    seq_snaps, seq_counts, seq_bare = kernel_sequence
    for f in range(1, N_FRAMES + 1):
        _same(snaps[f - 1], off_snaps[f - 1], f"{form} frame {f} against rt_gbuffer_reuse(0)")
        _same(snaps[f - 1], seq_snaps[f - 1], f"{form} frame {f} against frame_by_kernels")
    # the count rises exactly at the first frame of an epoch and by the bare rt_raycast; with the look-ahead on, a change may
    # throw one look-ahead trace away
    slack = 0 if form == "headline" else 1
    assert bare[1] == bare[0] + 1 and off_bare[1] == off_bare[0] + 1 and seq_bare[1] == seq_bare[0] + 1
    prev = 0
    for f, n in enumerate(counts, start=1):
        rise = n - prev - (1 if f == 14 else 0)  # frame 14's interval holds the bare rt_raycast
        if f in CHANGES:
            assert 1 <= rise <= 1 + slack, (form, f, counts)
        else:
            assert rise == 0, (form, f, counts)
        prev = n
    # reuse off: every frame traces (the look-ahead traces the next frame's rays beside this one: one launch per frame either way)
    prev = 0
    for f, n in enumerate(off_counts, start=1):
        assert n - prev - (1 if f == 14 else 0) >= 1, (form, f, off_counts)
        prev = n
    assert all(b - a == (2 if f == 14 else 1) for f, (a, b) in enumerate(zip([0] + seq_counts[:-1], seq_counts), start=1)), seq_counts


def test_frames_with_walk_counters_trace_and_the_frames_after_them_reuse(api, world):
    tune = ((api.Tune.SPEC, 0), (api.Tune.TAIL, 0))
    r, off = _renderer(api, world, tune), _renderer(api, world, tune, reuse=False)
    counts = []
    for f in range(1, 8):
        if f == 3:
            r.walk_stats_enable(True)
        r.frame(f)
        off.frame(f)
        if f == 5:
            ws = r.walk_stats()
            r.walk_stats_enable(False)
            assert ws["raycast"]["reference_rays"] == W * H * 3 and ws["raycast"]["walked"] == W * H * 3, ws
        _same(_snapshot(api, r), _snapshot(api, off), f"frame {f}")
        counts.append(r.primary_launches())
    assert counts == [1, 1, 2, 3, 4, 4, 4], counts
    r.close()
    off.close()


def test_timed_frames_reuse_and_their_parts_sum_to_the_frame(api, world):
    r = _renderer(api, world, ((api.Tune.WS_PRIMARY, 0), (api.Tune.WS, 1), (api.Tune.FUSE_RAYCAST, -1)))  # as the round-6 test: the one-launch form at this size
    r.timing_enable(True)
    for f in range(1, 7):
        r.frame(f)
        t = r.timing()
        parts = sum(t[k] for k in ("clear", "raycast", "generate_candidate", "spatial0", "spatial1", "spatial2", "resolve", "tone_mapping"))
        print(f, t)
        assert abs(parts - t["frame"]) <= 0.02 * t["frame"] + 0.005, (parts, t)
        assert r.stage0_one_launch()  # what a tracing frame would run under this tuning
        if f >= 2:
            assert t["raycast"] < 0.25 * t["generate_candidate"], t  # the empty bracket where the raycast launch would be
    assert r.primary_launches() == 1
    r.close()


def test_strip_contexts_refuse_and_trace_every_frame(api, world):
    from cedec_2024_rt_amd.types import bench_options

    r = api.Renderer(W, H, rows=(0, 38), halo=38)
    with pytest.raises(api.RtError) as e:
        r.gbuffer_reuse(True)
    assert f"error {RT_ERR_UNSUPPORTED}:" in str(e.value), str(e.value)
    r.gbuffer_reuse(False)  # allowed: it is what a strip does
    r.set_scene(world["A"])
    r.lookat(world["eye"], world["at"])
    r.set_options(bench_options())
    passes = int(r.options()["spatial_resampling_passes"][0])
    prev = 0
    for f in range(1, 5):
        for st in range(passes + 2):
            r.frame_stage(f, st)  # the halo rows are never filled: the image is no frame, the launches are a strip's
        n = r.primary_launches()
        assert n - prev >= 1, (f, prev, n)
        prev = n
    r.sync()
    r.close()


def test_script_a_first_ten_frames_equal_the_oracle(api, oracle, world):
    from cedec_2024_rt_amd.types import bench_options  # noqa: F401

    snaps = _run_a(api, world, "headline")[True][0]
    oracle.set_math_mode(oracle.MATH_PORTABLE)
    st = oracle.new_state(W, H)
    opt = oracle.bench_options()
    sc = oracle.Scene(world["A"], use_bvh=True)
    eye, at = world["eye"], world["at"]
    for f in range(1, 11):
        if f == 5:
            eye, at = EYE2, AT2
        if f == 8:
            sc = oracle.Scene(world["B"], use_bvh=True)
        rg = oracle.raygen_lookat(eye, at, (0, 1, 0), FOVY, W, H)
        sc.frame(W, H, f, rg, np.asarray(eye, np.float32), opt, st)
        acc = snaps[f - 1]["acc"]
        assert _eq_bits(acc, st["accum"].reshape(acc.shape)), (f, int((acc != st["accum"].reshape(acc.shape)).any(axis=1).sum()))
        assert np.array_equal(snaps[f - 1]["pix"].reshape(H, W, 4), st["pixels"]), f
