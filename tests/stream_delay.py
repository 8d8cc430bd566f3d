"""Stream ordering under injected delays: scripts, plans and the runner of tests/test_gpu_stream_order.py.

A frame of the library is work on four streams of its own (main, look-ahead, tail, second lane) tied together by events. On an idle
GPU short kernels run close to launch order, so a missing wait reads the right data by luck. rt_wire_delay parks ONE stream for a
time many times a frame while the others run on: every consumer on another stream that lacks its edge then runs before its
producer, and the bytes differ. With every edge present they cannot differ, so the assertion is bit equality.

* a SCRIPT is a list of API calls (steps) with checkpoints where buffers are downloaded;
* a PLAN says for every gap between two steps which of the streams "main", "tail", "lane" are held there;
* run() executes a script under a plan and a stream mode and returns the downloads;
* the REFERENCE run of a script has no plan, the context's own stream and rt_sync after every call.

Everything above the runner is plain data: tests/test_stream_delay_cpu.py checks the plans without a GPU.
"""
import time
import zlib
from collections import namedtuple

import numpy as np

STREAMS = ("main", "tail", "lane")
SLOT = {"main": 0, "tail": 1, "lane": 2}  # one d_wire slot per stream: no stamp overwrites one a pending wait will read
PLANS = ("none", "main_every_gap", "tail_every_gap", "lane_every_gap", "main_and_tail_alternating", "random_1", "random_2")
STREAM_MODES = ("own", "caller", "null", "switching")
NS_MIN, NS_MAX = 1_000_000, 4_000_000  # the library refuses more than 5 ms
FRAMES = 12  # the buffer rotation has a period of several frames

ROOM_EYE, ROOM_AT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)

# op: a name of OPS; args: its arguments; lane_ok: whether the gap BEFORE this step may hold the second lane (rt_lane(ctx, 1) starts the
# stage's lane, after which rt_frame_stage_fork is an error: between a stage's _begin and its _fork the lane cannot be held)
Step = namedtuple("Step", "op args lane_ok")
Script = namedtuple("Script", "name W H scene options setup steps oracle_frames rows halo", defaults=(None, 0))  # rows: a strip context's


def S(op, *args, lane_ok=True):
    return Step(op, tuple(args), lane_ok)


# ------------------------------------------------------------------------------------------------ plans
def n_gaps(script):
    return len(script.steps) - 1


def allowed(script, gap):
    """the streams that may be held in the gap before step gap + 1"""
    return STREAMS if script.steps[gap + 1].lane_ok else STREAMS[:2]


def plan(name, script):
    """per gap, the frozenset of streams held there"""
    n = n_gaps(script)
    if name == "none":
        held = [() for _ in range(n)]
    elif name.endswith("_every_gap"):
        held = [(name[: -len("_every_gap")],) for _ in range(n)]
    elif name == "main_and_tail_alternating":
        held = [(("main", "tail")[g % 2],) for g in range(n)]
    elif name.startswith("random_"):
        # a random subset in every gap; the draw depends on the seed and the script alone
        rng = np.random.default_rng([int(name[len("random_"):]), zlib.crc32(script.name.encode())])
        held = [tuple(s for s, on in zip(STREAMS, rng.integers(0, 2, size=3)) if on) for _ in range(n)]
    else:
        raise ValueError(f"unknown plan {name!r}")
    return [frozenset(s for s in h if s in allowed(script, g)) for g, h in enumerate(held)]


def delay_ns(frame_seconds):
    """the hold for a size whose undelayed frame takes `frame_seconds`: 8 frames, within [1 ms, 4 ms]; None = the image is too large
    for this test (shrink it, the cap stays)"""
    ns = int(8 * frame_seconds * 1e9)
    if ns > NS_MAX:
        return None
    return max(ns, NS_MIN)


# ------------------------------------------------------------------------------------------------ scripts
def _frames(first, last, clear_at=()):
    return [S("frame", f, f in clear_at) for f in range(first, last + 1)]


def _frame_script(name, W=96, H=54, scene="room", setup=(), frames=FRAMES, **options):
    steps = _frames(1, 7) + [S("checkpoint")] + _frames(8, frames) + [S("checkpoint")]
    return Script(name, W, H, scene, options, tuple(setup), tuple(steps), frames)


def frame_scripts():
    """a. rt_frame back to back, every variant a script of its own. 480x270 is the size of the existing back-to-back tests (its
    kernels are several rounds of wavefronts); the forms that do not depend on the size run at 96x54."""
    t = lambda key, v: ("tuning", (key, v))  # noqa: E731
    s = [
        _frame_script("defaults_480x270", 480, 270, "blocks", setup=[("expect_tuning", ("SPEC", -1)), ("expect_tuning", ("TAIL", -1))]),
        _frame_script("defaults", setup=[("expect_tuning", ("SPEC", -1)), ("expect_tuning", ("TAIL", -1))]),
        _frame_script("spec1", setup=[t("SPEC", 1), ("expect_tuning", ("SPEC", 1))]),
        _frame_script("spec0_tail0", setup=[t("SPEC", 0), t("TAIL", 0), ("expect_tuning", ("SPEC", 0)), ("expect_tuning", ("TAIL", 0))]),
        _frame_script("spec_free1", setup=[t("SPEC_FREE", 1), ("expect_tuning", ("SPEC_FREE", 1))]),
        _frame_script("fuse_tonemap0", setup=[t("FUSE_TONEMAP", 0), ("expect_tuning", ("FUSE_TONEMAP", 0))]),
        # the one-launch stage 0 is the candidates' work-sharing walk behind a plain primary walk; a launch this small takes the
        # work-sharing primary walk by default and with it two launches
        _frame_script("one_launch", setup=[t("FUSE_RAYCAST", 1), t("WS_PRIMARY", 0), ("expect_one_launch", (True,))]),
        _frame_script("two_launches", setup=[t("FUSE_RAYCAST", 0), ("expect_one_launch", (False,))]),
        _frame_script("gbuffer_reuse1", setup=[("gbuffer_reuse", (True,)), ("expect_primary_launches", (1, 1))]),
        _frame_script("gbuffer_reuse0", setup=[("gbuffer_reuse", (False,)), ("expect_primary_launches", (FRAMES + 1, FRAMES + 1))]),  # frame 1 and twelve look-aheads: SPEC = 0 would make it twelve
        _frame_script("shadowed", use_shadowed_target_function=1),
    ]
    # the pass count changes which buffer the tail reads and which join_tail_for guards
    s += [_frame_script(f"passes{p}", spatial_resampling_passes=p) for p in (0, 1, 2, 4)]
    return s


def staged_script():
    """b. the staged API as the strip driver uses it, on one whole-frame context: every stage runs its upper rows on the main stream
    and, behind a fork, its lower rows on the second lane; stage 0 is split into its parts 1 (primary rays, all rows) and 2 (candidates)
    with the fork between them."""
    H, cut, passes = 54, 23, 1  # one pass: 193 gaps, under 0.3 s of holds per stream up to 1.55 ms (a 96x54 frame of 190 us)
    steps = []
    for f in range(1, FRAMES + 1):
        for st in range(passes + 2):
            steps.append(S("stage_begin", f, st))
            if st == 0:
                steps.append(S("stage_run_part", f, 0, 1, 0, H, lane_ok=False))
                steps.append(S("stage_fork", lane_ok=False))
                steps.append(S("stage_run_part", f, 0, 2, 0, cut))
                steps.append(S("stage_run_async", f, 0, 2, cut, H))
            else:
                steps.append(S("stage_run_part", f, st, 0, 0, cut, lane_ok=False))
                steps.append(S("stage_fork", lane_ok=False))
                steps.append(S("stage_run_async", f, st, 0, cut, H))
            steps.append(S("stage_end", st))
        if f == 7:
            steps.append(S("checkpoint"))
    steps.append(S("checkpoint"))
    return Script("staged_two_lanes", 96, H, "room", dict(spatial_resampling_passes=passes), (), tuple(steps), FRAMES)


BUF_NAMES = ("VISIBILITY", "RES_0", "RES_1", "RES_TEMPORAL", "ACCUMULATION", "PIXELS")
FOREIGN = (
    ["clear", "raycast", "generate_candidate", "temporal_resampling", "save_temporal_reservoir", "spatial_resampling", "resolve",
     "tone_mapping"]
    + [f"upload_{b}" for b in BUF_NAMES if b != "PIXELS"]  # the pixels are written by the library alone
    + [f"download_{b}" for b in BUF_NAMES]
    + ["download_DENOISED", "download_DENOISE_GUIDE", "download_DENOISE_HISTORY"]  # F = the denoiser that writes it, then the download
    + ["path_trace_7", "path_trace_6", "denoise", "denoise_temporal", "scene_update", "camera_orbit", "options_set",
       "light_sampling", "temporal_reprojection", "temporal_motion", "occluder_hints", "gbuffer_reuse"]
)


def foreign_script(name):
    """c. one call F of another kind between unsynchronised frames: frames 1-3, F, frames 4-6, F again, frames 7-8. What F does is what
    the reference run makes of it. A camera move is followed by a frame that clears first."""
    clear_at = (4, 7) if name == "camera_orbit" else ()
    options = {}
    if name.startswith("upload_"):
        # accumulating frames: without them the next frame's resolve overwrites the accumulation, and neither an uploaded accumulation nor
        # a resolve that read a reservoir buffer on the wrong side of its upload would reach the checkpoint
        clear_at, options = (1,), dict(accumulate=1)
    steps = _frames(1, 3) + [S("foreign", name, 0)] + _frames(4, 6, clear_at) + [S("foreign", name, 1)] + _frames(7, 8, clear_at) + [S("checkpoint")]
    return Script(f"foreign_{name}", 96, 54, "room", options, (), tuple(steps), None)


def foreign_scripts():
    return [foreign_script(n) for n in FOREIGN]


STRIP_W, STRIP_H, STRIP_HALO, STRIP_PLANS = 96, 300, 87, ("none", "main_every_gap", "tail_every_gap", "main_and_tail_alternating", "random_1", "random_2")

# on a strip context (the middle strip of 96x300 in three, halo 87) the frames are rt_frame_stage calls with nothing exchanged: the halo
# rows hold what the foreign calls put there, and the neighbours' shaded flags are the strip's own bands' (unpacked once, before the script:
# rt_halo_mark_sides asks for them).
STRIP_ROWS = (100, 200)
STRIP_FOREIGN = ["halo_pack", "halo_unpack", "halo_flags_pack", "halo_flags_unpack", "copy_parts", "halo_mark_sides", "halo_mark_sides_two_streams",
                 "halo_pack_sparse_ranges", "halo_unpack_sparse_ranges"]


def strip_foreign_script(name):
    fr = lambda a, b: [S("strip_frame", f) for f in range(a, b + 1)]  # noqa: E731
    steps = fr(1, 3) + [S("strip_foreign", name, 0)] + fr(4, 6) + [S("strip_foreign", name, 1)] + fr(7, 8) + [S("checkpoint")]
    return Script(f"strip_foreign_{name}", STRIP_W, STRIP_H, "room", {}, (), tuple(steps), None, STRIP_ROWS, STRIP_HALO)


def strip_foreign_scripts():
    return [strip_foreign_script(n) for n in STRIP_FOREIGN]


def strips_script(dense):
    """d. three strips on the LOCAL hub: the steps are the sweeps of rt_mg_frame_step over the ranks (as many as the driver asks for:
    the plan repeats after 64), each rank's main and tail held between them. As a script of the single context it is twelve frames."""
    s = _frame_script("strips_dense" if dense else "strips_sparse", STRIP_W, STRIP_H)
    sweeps = tuple(S("mg_sweep", lane_ok=False) for _ in range(65))
    return s, s._replace(steps=sweeps)


def all_scripts():
    """the scripts of one context (the strips' plans are checked beside them)"""
    return frame_scripts() + [staged_script()] + foreign_scripts() + strip_foreign_scripts()


# ------------------------------------------------------------------------------------------------ the hold
def hold(r, where, ns):
    """park one stream of the context for `ns`: stamp, then wait, both on that stream. main = the context's current stream, whatever
    it is; tail = the tail stream, through rt_set_stream and back to the stream rt_get_stream named before; lane = between rt_lane(1)
    and rt_lane(0)."""
    slot = SLOT[where]
    if where == "main":
        r.wire_delay(0, slot, 0)
        r.wire_delay(1, slot, ns)
    elif where == "tail":
        before = r.get_stream()
        r.set_stream(r.side_stream(0))
        try:
            r.wire_delay(0, slot, 0)
            r.wire_delay(1, slot, ns)
        finally:
            r.set_stream(before)
    elif where == "lane":
        r.lane(True)
        try:
            r.wire_delay(0, slot, 0)
            r.wire_delay(1, slot, ns)
        finally:
            r.lane(False)
    else:
        raise ValueError(where)


# ------------------------------------------------------------------------------------------------ the runner
class _Env:
    """what the ops of one run share"""

    def __init__(self, api, script, r, tris):
        self.api, self.script, self.r, self.tris = api, script, r, tris
        self.out = []      # (label, array) in script order
        self.step = 0
        self.denoised = self.denoised_temporal = False
        self.streams = None  # switching: the streams the frames rotate over, and the one in use
        self.cur = 0
        self.keep = []
        self.dev = {}      # a strip script's device buffers (torch tensors)
        self.uploads = None  # what the upload_* calls upload: None = download it here and record it (the reference run)
        self.recorded = {}


def _scene(api, name):
    from cedec_2024_rt_amd import scenes

    if name == "blocks":
        return scenes.make_blocks_restir(), scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT
    return scenes.make_quad_room(), ROOM_EYE, ROOM_AT


def _download(e, buf, name):
    e.out.append((f"step {e.step} {name}", e.r.download(buf)))


def _checkpoint(e):
    a = e.api
    _download(e, a.RT_BUF_ACCUMULATION, "accumulation")
    _download(e, a.RT_BUF_PIXELS, "pixels")
    _download(e, a.RT_BUF_RES_TEMPORAL, "RES_TEMPORAL")
    if e.script.rows:  # a strip: the halo rows of every reservoir buffer are what the halo calls write
        _download(e, a.RT_BUF_RES_0, "RES_0")
        _download(e, a.RT_BUF_RES_1, "RES_1")
        e.r.sync()
        for k, t in sorted(e.dev.items()):
            e.out.append((f"step {e.step} device buffer {k}", t.cpu().numpy().reshape(-1, 1)))
    if e.denoised or e.denoised_temporal:
        _download(e, a.RT_BUF_DENOISED, "denoised")
    if e.denoised:
        _download(e, a.RT_BUF_DENOISE_GUIDE, "denoise guide")
    if e.denoised_temporal:
        _download(e, a.RT_BUF_DENOISE_HISTORY, "denoise history")


def _switch(e):
    """the next of the streams the frames rotate over. Ordering the switch is the caller's duty: an event recorded on the stream it
    leaves, waited for on the stream it enters."""
    import torch

    leave = e.streams[e.cur]
    e.cur = (e.cur + 1) % len(e.streams)
    enter = e.streams[e.cur]
    ev = torch.cuda.Event()
    ev.record(leave)
    enter.wait_event(ev)
    e.keep.append(ev)
    e.r.set_stream(enter.cuda_stream)


def _frame(e, f, clear=False):
    if e.streams:
        _switch(e)
    e.r.frame(f, clear)


def _strip_frame(e, f):
    if e.streams:
        _switch(e)
    for st in range(int(e.r.options()["spatial_resampling_passes"][0]) + 2):
        e.r.frame_stage(f, st)


def _neighbour_flags(e):
    """a G-buffer of the current camera, and as the neighbours' shaded flags the strip's own bands': all halo rows of both sides under the
    current epoch, which rt_halo_mark_sides asks for"""
    r, (r0, r1), n = e.r, e.script.rows, e.script.halo
    r.raycast()
    for own, halo_row in ((r0, r.local_row0), (r1 - n, r1)):
        r.halo_flags_pack(own, n, e.dev["flags"].data_ptr())
        r.halo_flags_unpack(halo_row, n, e.dev["flags"].data_ptr())


def _strip_foreign(e, name, k):
    """the k-th application of a halo call on the strip context; rows: the strip's own top band, its own bottom band and its two halos"""
    a, r, n = e.api, e.r, e.script.halo
    (r0, r1), lo = e.script.rows, e.r.local_row0
    if name == "halo_pack":
        r.halo_pack(a.RT_RES_TEMPORAL, (r0, r1 - n)[k], n, e.dev["records"].data_ptr())
    elif name == "halo_unpack":  # what a neighbour would send: here the strip's own band, into the halo beside it
        r.halo_pack(a.RT_RES_TEMPORAL, (r0, r1 - n)[k], n, e.dev["records"].data_ptr())
        r.halo_unpack(a.RT_RES_TEMPORAL, (lo, r1)[k], n, e.dev["records"].data_ptr())
    elif name == "halo_flags_pack":
        r.halo_flags_pack((r0, r1 - n)[k], n, e.dev["flags"].data_ptr())
    elif name == "halo_flags_unpack":
        r.halo_flags_pack((r0, r1 - n)[k], n, e.dev["flags"].data_ptr())
        r.halo_flags_unpack((lo, r1)[k], n, e.dev["flags"].data_ptr())
    elif name in ("halo_mark_sides", "halo_mark_sides_two_streams", "halo_pack_sparse_ranges", "halo_unpack_sparse_ranges"):
        import ctypes as C

        passes = int(r.options()["spatial_resampling_passes"][0])
        frame = (4, 7)[k]  # the marks of the frame that follows
        words = r.halo_bitmap_words(n)  # per pass and side; both sides in one allocation, side 0 first (one clear)
        side = [e.dev["marks"].data_ptr() + 4 * passes * words * s for s in (0, 1)]
        r._ck(r.L.rt_halo_mark_sides(r.h, frame, 0, passes, C.c_void_p(side[0]), C.c_void_p(side[1])))
        if name == "halo_mark_sides_two_streams" and k == 1:
            # under a new camera the shaded bits are rebuilt by the mark on the main stream: the mark on the tail stream must not read the old ones
            r.orbit(35.0, -12.0)
            _neighbour_flags(e)
            r._ck(r.L.rt_halo_mark_sides(r.h, frame, 0, passes, C.c_void_p(side[0]), C.c_void_p(side[1])))
        if name == "halo_mark_sides_two_streams":
            # as the strip driver marks: on the tail stream, from the shaded bits a mark on the main stream has built (ev_mark_bits)
            side_t = [e.dev["marks_tail"].data_ptr() + 4 * passes * words * s for s in (0, 1)]
            before = r.get_stream()
            r.set_stream(r.side_stream(0))
            try:
                r._ck(r.L.rt_halo_mark_sides(r.h, frame, 0, passes, C.c_void_p(side_t[0]), C.c_void_p(side_t[1])))
            finally:
                r.set_stream(before)
        if name.endswith("sparse_ranges"):
            # pass 0's bitmap of each side: what the neighbour on that side would ask of this strip's band beside it (the mirror
            # transport's exchange); a list holds at most every record of its 87 rows
            nr = (C.c_int * 2)(n, n)
            bms = (C.c_void_p * 2)(*side)
            lists = (C.c_void_p * 2)(e.dev["list0"].data_ptr(), e.dev["list1"].data_ptr())
            r._ck(r.L.rt_halo_pack_sparse_ranges(r.h, a.RT_RES_TEMPORAL, 2, (C.c_int * 2)(r0, r1 - n), nr, bms, lists))
            if name == "halo_unpack_sparse_ranges":
                r._ck(r.L.rt_halo_unpack_sparse_ranges(r.h, a.RT_RES_TEMPORAL, 2, (C.c_int * 2)(lo, r1), nr, bms, lists))
    elif name == "copy_parts":
        import ctypes as C

        src, dst = e.dev["pattern"], e.dev["copy"]
        off, nbytes = ((0, 4099), (5000, 1000))[k], ((4099, 901), (1000, 37))[k]  # 16-byte, 4-byte and unaligned parts
        ps = (C.c_void_p * 2)(*[src.data_ptr() + o for o in off])
        pd = (C.c_void_p * 2)(*[dst.data_ptr() + o for o in off])
        nb = (C.c_size_t * 2)(*nbytes)
        r._ck(r.L.rt_copy_parts(r.h, 2, ps, pd, nb))
    else:
        raise ValueError(name)


def _foreign(e, name, k):
    """the k-th (0, 1) application of foreign call `name`"""
    a, r = e.api, e.r
    if name.startswith("upload_"):
        # what is uploaded is what the buffer holds, changed where that is allowed: the upload is then valid whatever the frames left there
        # (a G-buffer of this camera, reservoirs with M in range). The synchronised run downloads and records it; a delayed run uploads
        # the recorded bytes with no call in front of rt_upload, which is then the first to meet a parked tail.
        buf = getattr(a, "RT_BUF_" + name[len("upload_"):])
        if e.uploads is None:
            data = r.download(buf)
            if buf == a.RT_BUF_ACCUMULATION:
                data = (data * np.float32(0.5)).astype(np.float32)
            elif buf != a.RT_BUF_VISIBILITY:
                data["ucw"] = (data["ucw"] * np.float32(0.5)).astype(np.float32)  # other bytes than the buffer holds: a resolve that reads them shows
            e.recorded[(name, k)] = data
        else:
            data = e.uploads[(name, k)]
        r.upload(buf, data)
    elif name in ("download_DENOISED", "download_DENOISE_GUIDE", "download_DENOISE_HISTORY"):
        if k == 0 and name == "download_DENOISE_HISTORY":
            r._ck(r.L.rt_denoise_temporal(r.h, None, None))
            e.denoised_temporal = True
        elif k == 0:
            r._ck(r.L.rt_denoise(r.h, None))
            e.denoised = True
        else:
            _download(e, getattr(a, "RT_BUF_" + name[len("download_"):]), name)
    elif name.startswith("download_"):
        _download(e, getattr(a, "RT_BUF_" + name[len("download_"):]), name)
    elif name == "clear":
        r.clear()
    elif name == "raycast":
        r.raycast()
    elif name == "generate_candidate":
        r.generate_candidate(100 + k, a.RT_RES_0)
    elif name == "temporal_resampling":
        r.temporal_resampling(100 + k, a.RT_RES_TEMPORAL, a.RT_RES_0)
    elif name == "save_temporal_reservoir":
        r.save_temporal_reservoir(a.RT_RES_0, a.RT_RES_TEMPORAL)
    elif name == "spatial_resampling":
        r.spatial_resampling(100 + k, 0, a.RT_RES_0, a.RT_RES_1)
    elif name == "resolve":
        r.resolve(a.RT_RES_1)
    elif name == "tone_mapping":
        r.tone_mapping()
    elif name == "path_trace_7":
        r.path_trace(7, 1 + k)
    elif name == "path_trace_6":
        r.path_trace(6, 0)
    elif name == "denoise":
        r._ck(r.L.rt_denoise(r.h, None))
        e.denoised = True
    elif name == "denoise_temporal":
        r._ck(r.L.rt_denoise_temporal(r.h, None, None))
        e.denoised_temporal = True
    elif name == "scene_update":
        from cedec_2024_rt_amd import scenes

        mask = np.zeros(len(e.tris), bool)
        mask[-4:] = True
        e.tris = scenes.move_triangles(e.tris, mask, (0.0, 0.03125 * (k + 1), 0.0))
        r.update_scene(e.tris[-4:], first=len(e.tris) - 4)
    elif name == "camera_orbit":
        r.orbit(0.125 * (k + 1), 0.0625)
    elif name == "options_set":
        from cedec_2024_rt_amd.types import bench_options

        r.set_options(bench_options(spatial_resampling_passes=(2, 1)[k], **e.script.options))
    elif name == "light_sampling":
        r.light_sampling(("power", "uniform")[k])
    elif name == "temporal_reprojection":
        r.temporal_reprojection(k == 0)
    elif name == "temporal_motion":
        r.temporal_motion(k == 0)
    elif name == "occluder_hints":
        r.occluder_hints(k == 1)
    elif name == "gbuffer_reuse":
        r.gbuffer_reuse(k == 1)
    else:
        raise ValueError(name)


OPS = {
    "frame": _frame,
    "checkpoint": _checkpoint,
    "foreign": _foreign,
    "strip_frame": _strip_frame,
    "strip_foreign": _strip_foreign,
    "stage_begin": lambda e, f, st: e.r.frame_stage_begin(f, st),
    "stage_run_part": lambda e, f, st, part, r0, r1: e.r.frame_stage_run_part(f, st, part, r0, r1),
    "stage_fork": lambda e: e.r.frame_stage_fork(),
    "stage_run_async": lambda e, f, st, part, r0, r1: e.r.frame_stage_run_async(f, st, part, r0, r1),
    "stage_end": lambda e, st: e.r.frame_stage_end(st),
}


def _setup(e, op, args):
    """before the first step: tuning and switches. The expect_* entries are checked by _verify_form after the run."""
    r = e.r
    if op == "tuning":
        r.tuning(getattr(e.api.Tune, args[0]), args[1])
    elif op == "gbuffer_reuse":
        r.gbuffer_reuse(args[0])
    elif not op.startswith("expect_"):
        raise ValueError(op)


def _verify_form(e, one_launch_after_frame1):
    """the form named in the case is the one that ran (host state: asking does not wait for anything)"""
    r = e.r
    for op, args in e.script.setup:
        if op == "expect_tuning":
            got = r.tuning_get(getattr(e.api.Tune, args[0]))
            assert got == args[1], f"{e.script.name}: rt_tuning {args[0]} is {got}, the case wants {args[1]}"
        elif op == "expect_one_launch":
            assert one_launch_after_frame1 == args[0], f"{e.script.name}: stage 0 of frame 1 ran as {'one launch' if one_launch_after_frame1 else 'two launches'}"
        elif op == "expect_primary_launches":
            assert args[0] <= r.primary_launches() <= args[1], f"{e.script.name}: {r.primary_launches()} launches traced primary rays, the case wants {args}"


Run = namedtuple("Run", "out seconds main_holds recorded")


def new_context(api, script, lib_path=None):
    from cedec_2024_rt_amd.types import bench_options

    tris, eye, at = _scene(api, script.scene)
    r = api.Renderer(script.W, script.H, rows=script.rows, halo=script.halo, lib_path=lib_path)
    e = _Env(api, script, r, tris)
    if script.rows:
        import torch

        # device memory the halo calls write to and read from, sized by the library's own size functions
        e.dev = dict(records=torch.zeros(r.halo_bytes(script.halo), dtype=torch.uint8, device="cuda"),
                     flags=torch.zeros(r.halo_flags_bytes(script.halo), dtype=torch.uint8, device="cuda"),
                     pattern=(torch.arange(8192, device="cuda") % 251).to(torch.uint8), copy=torch.zeros(8192, dtype=torch.uint8, device="cuda"))
        if "mark" in script.name or "sparse" in script.name:
            words = 2 * 8 * r.halo_bitmap_words(script.halo)  # both sides, up to 8 passes
            e.dev.update(marks=torch.zeros(words, dtype=torch.int32, device="cuda"), marks_tail=torch.zeros(words, dtype=torch.int32, device="cuda"),
                         list0=torch.zeros(r.halo_bytes(script.halo), dtype=torch.uint8, device="cuda"),
                         list1=torch.zeros(r.halo_bytes(script.halo), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()  # the context's streams do not wait for torch's
    for op, args in script.setup:
        _setup(e, op, args)
    r.set_scene(tris)
    r.lookat(eye, at)
    r.set_options(bench_options(**script.options))
    r.wire_delay(0, 7, 0)  # the stamps' memory is allocated at the first call: not in the middle of the script
    if script.rows:
        _neighbour_flags(e)
    r.sync()
    return e


def run(api, script, plan_name="none", stream_mode="own", ns=0, sync_every_call=False, lib_path=None, uploads=None):
    """the checkpoint downloads of `script` with the streams of plan `plan_name` held for `ns` in its gaps. stream_mode: "own", "caller"
    (a torch stream through rt_set_stream), "null" (HIP's null stream) or "switching" (the frames rotate over two caller streams and
    the context's own). The last step of every script is a checkpoint: the run ends with rt_download alone, no host sync of the
    caller's."""
    held = plan(plan_name, script)
    e = new_context(api, script, lib_path)
    e.uploads = uploads
    r = e.r
    try:
        if stream_mode != "own":
            import torch

            if stream_mode == "caller":
                e.keep.append(torch.cuda.Stream())
                r.set_stream(e.keep[0].cuda_stream)
                assert r.get_stream() == e.keep[0].cuda_stream
            elif stream_mode == "null":
                r.set_stream(0)
                assert r.get_stream() == 0
            elif stream_mode == "switching":
                e.streams = [torch.cuda.ExternalStream(r.get_stream()), torch.cuda.Stream(), torch.cuda.Stream()]
            else:
                raise ValueError(stream_mode)
        one_launch = None
        main_holds = 0
        t0 = time.perf_counter()
        for i, st in enumerate(script.steps):
            if i > 0:
                for where in STREAMS:  # a fixed order: the plan is a set
                    if where in held[i - 1]:
                        hold(r, where, ns)
                        main_holds += where == "main"
            e.step = i
            OPS[st.op](e, *st.args)
            if one_launch is None and st.op in ("frame", "strip_frame"):
                one_launch = r.stage0_one_launch()
            if sync_every_call:
                r.sync()
        seconds = time.perf_counter() - t0
        _verify_form(e, one_launch)
        return Run(e.out, seconds, main_holds, e.recorded)
    finally:
        r.close()


def reference(api, script):
    """no plan, the context's own stream, rt_sync after every call: (downloads, what its upload_* calls uploaded)"""
    ref = run(api, script, sync_every_call=True)
    return ref.out, ref.recorded


def differences(want, got, W):
    """[] if the downloads are the same bytes, else one line per differing download that names pixels"""
    bad = []
    if [n for n, _ in want] != [n for n, _ in got]:
        return [f"downloads differ: {[n for n, _ in want]} / {[n for n, _ in got]}"]
    for (name, a), (_, b) in zip(want, got):
        a8 = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
        b8 = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
        px = np.nonzero((a8 != b8).any(axis=1))[0]
        if len(px):
            first = ", ".join(f"({int(p) % W}, {int(p) // W})" for p in px[:4])
            bad.append(f"{name}: {len(px)} of {len(a)} pixels differ, first at (x, y) = {first}")
    return bad
