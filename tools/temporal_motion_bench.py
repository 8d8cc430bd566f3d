"""GPU. What rt_temporal_motion costs where geometry moves every frame: two contexts in one process over the bench stand-in, both with
rt_temporal_reprojection on, the toggle off and on; before every frame from the second on both get the same rt_scene_update, a span of
non-emissive triangles moved up and down by --dy in turn (the same float add as scenes.move_triangles). The span is the window of --count
triangles without an emitter that the most pixels of the first frame show. Their frames alternate, each timed with HIP events
(rt_timing). Reports the means, the paired per-frame difference of stage 0 and of the frame, and from one more frame that is not timed
the share of shaded pixels on moved triangles and of those that found a valid history (rt_temporal_motion_stats). Not a parity run: the
two images differ by construction.
  python tools/temporal_motion_bench.py [WxH] [--count N] [--dy UNITS] [--json FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cedec_2024_rt_amd import api, scenes  # noqa: E402
from cedec_2024_rt_amd.types import bench_options  # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


out_json = _opt("--json", None)
COUNT = int(_opt("--count", "4096"))
DY = float(_opt("--dy", "0.5"))
args = sys.argv[1:]
W, H = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
WARMUP, FRAMES = 8, 96
tris = scenes.make_blocks_restir()
names = ("clear", "raycast", "generate_candidate", "spatial0", "spatial1", "spatial2", "resolve", "tone_mapping", "frame")
ctx = {}
for label, on in (("off", False), ("on", True)):
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options())
    r.temporal_reprojection(True)
    r.temporal_motion(on)
    r.timing_enable(True)
    ctx[label] = r
# the span: pixels per triangle of the first frame's primary rays, summed over windows of COUNT triangles without an emitter
r = ctx["off"]
r.raycast()
idx = r.download(api.RT_BUF_VISIBILITY)["index"]
seen = np.bincount(idx[idx >= 0], minlength=len(tris)).astype(np.int64)
emissive = (tris["emissive"] > 0).any(axis=1).astype(np.int64)
c_seen, c_emi = np.concatenate([[0], np.cumsum(seen)]), np.concatenate([[0], np.cumsum(emissive)])
COUNT = min(COUNT, len(tris))
win = c_seen[COUNT:] - c_seen[:-COUNT]
win[(c_emi[COUNT:] - c_emi[:-COUNT]) > 0] = -1
FIRST = int(np.argmax(win))
assert win[FIRST] > 0, "no window of %d triangles without an emitter is visible" % COUNT
print("moving triangles [%d, %d): %d of %d pixels show them" % (FIRST, FIRST + COUNT, win[FIRST], W * H), flush=True)
mask = np.zeros(len(tris), bool)
mask[FIRST:FIRST + COUNT] = True
cur = dict(off=tris, on=tris)
rows = dict(off=[], on=[])
upd = dict(off=[], on=[])


def step(label, f):
    import time
    r = ctx[label]
    if f > 1:
        cur[label] = scenes.move_triangles(cur[label], mask, (0.0, DY if f % 2 == 0 else -DY, 0.0))
        span = np.ascontiguousarray(cur[label][FIRST:FIRST + COUNT])
        t0 = time.perf_counter()
        r.update_scene(span, first=FIRST)
        if f > WARMUP:
            upd[label].append((time.perf_counter() - t0) * 1e3)
    r.frame(f)


for f in range(1, WARMUP + FRAMES + 1):
    for label in (("off", "on") if f % 2 else ("on", "off")):  # who goes first alternates too
        step(label, f)
        t = ctx[label].timing()
        if f > WARMUP:
            rows[label].append([t[k] for k in names])
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES, first=FIRST, count=COUNT, dy=DY, pixels_on_span=int(win[FIRST]), build_id=ctx["on"].build_id(),
              one_launch_stage0=bool(ctx["on"].stage0_one_launch()))
for label in ("off", "on"):
    a, u = np.array(rows[label]), np.array(upd[label])
    m, sd = a.mean(axis=0), a.std(axis=0, ddof=1)
    result[label] = dict(raycast_ms=float(m[1]), stage0_ms=float(m[2]), stage0_sd=float(sd[2]), frame_ms=float(m[8]), frame_sd=float(sd[8]),
                         scene_update_ms=float(u.mean()), scene_update_sd=float(u.std(ddof=1)))
    print("toggle %-3s stage 0 %.4f ms (sd %.4f)  frame %.4f ms (sd %.4f)  rt_scene_update %.4f ms (sd %.4f, host clock)" %
          (label, m[2], sd[2], m[8], sd[8], u.mean(), u.std(ddof=1)), flush=True)
# the two contexts see the same scenes, so frame f of one pairs with frame f of the other
d = np.array(rows["on"]) - np.array(rows["off"])
dm, dse = d.mean(axis=0), d.std(axis=0, ddof=1) / np.sqrt(len(d))
du = np.array(upd["on"]) - np.array(upd["off"])
result["paired_on_minus_off"] = dict(stage0_ms=float(dm[2]), stage0_se=float(dse[2]), frame_ms=float(dm[8]), frame_se=float(dse[8]),
                                     scene_update_ms=float(du.mean()), scene_update_se=float(du.std(ddof=1) / np.sqrt(len(du))))
result["paired_on_minus_off"]["per_kernel_ms"] = {k: [float(dm[i]), float(dse[i])] for i, k in enumerate(names)}
print("paired on - off: stage 0 %+.4f ms (standard error %.4f)  frame %+.4f ms (standard error %.4f)  rt_scene_update %+.4f ms (%.4f)" %
      (dm[2], dse[2], dm[8], dse[8], du.mean(), du.std(ddof=1) / np.sqrt(len(du))), flush=True)
r = ctx["on"]
r.timing_enable(False)
r.walk_stats_enable(True)
step("on", WARMUP + FRAMES + 1)
st = r.temporal_motion_stats()
r.walk_stats_enable(False)
result["stats"] = st
result["in_range_share"] = st["in_range"] / max(st["merged"], 1)
result["valid_share"] = st["valid"] / max(st["in_range"], 1)
print("shaded pixels %d, on moved triangles %.4f, valid histories among those %.4f" % (st["merged"], result["in_range_share"], result["valid_share"]))
print("on / off: stage 0 %.3fx, frame %.3fx" % (result["on"]["stage0_ms"] / result["off"]["stage0_ms"], result["on"]["frame_ms"] / result["off"]["frame_ms"]))
for c in ctx.values():
    c.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
