"""GPU. What rt_temporal_unbiased costs under a moving camera: two contexts in one process, both with rt_temporal_reprojection on, the
toggle off and the toggle on, orbit in step over the bench stand-in (one rt_camera_orbit per frame, so every frame traces its primary
rays and gathers its history by reprojection; with the toggle on stage 0 is the candidates' launch and k_temporal_unbiased); their
frames alternate, each timed with HIP events (rt_timing). Reports the means and the paired per-frame difference of stage 0, resolve
and the frame (the toggle-off context is the figure of tools/temporal_reproject_bench.py's mode on, measured in this run), and from
one more frame that is not timed the counters of rt_temporal_unbiased_stats and resolve's walk counters of both contexts. Not a parity
run: the two images differ by construction.
  python tools/temporal_unbiased_bench.py [WxH] [--dx PIXELS] [--json FILE]"""
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
DX = float(_opt("--dx", "4"))
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
    r.temporal_unbiased(on)
    r.timing_enable(True)
    ctx[label] = r
rows = dict(off=[], on=[])
for f in range(1, WARMUP + FRAMES + 1):
    for label in (("off", "on") if f % 2 else ("on", "off")):  # who goes first alternates too
        r = ctx[label]
        if f > 1:
            r.orbit(DX, 0.0)
        r.frame(f)
        t = r.timing()
        if f > WARMUP:
            rows[label].append([t[k] for k in names])
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES, orbit_dx=DX, build_id=ctx["on"].build_id(), one_launch_stage0=bool(ctx["on"].stage0_one_launch()))
for label in ("off", "on"):
    a = np.array(rows[label])
    m, sd = a.mean(axis=0), a.std(axis=0, ddof=1)
    result[label] = dict(raycast_ms=float(m[1]), stage0_ms=float(m[2]), stage0_sd=float(sd[2]), resolve_ms=float(m[6]), resolve_sd=float(sd[6]),
                         frame_ms=float(m[8]), frame_sd=float(sd[8]))
    print("toggle %-3s raycast bracket %.4f ms  stage 0 %.4f ms (sd %.4f)  resolve %.4f ms (sd %.4f)  frame %.4f ms (sd %.4f)"
          % (label, m[1], m[2], sd[2], m[6], sd[6], m[8], sd[8]), flush=True)
# the two contexts see the same cameras, so frame f of one pairs with frame f of the other: the view's frame-to-frame spread cancels
d = np.array(rows["on"]) - np.array(rows["off"])
dm, dse = d.mean(axis=0), d.std(axis=0, ddof=1) / np.sqrt(len(d))
result["paired_on_minus_off"] = dict(stage0_ms=float(dm[2]), stage0_se=float(dse[2]), resolve_ms=float(dm[6]), resolve_se=float(dse[6]),
                                     frame_ms=float(dm[8]), frame_se=float(dse[8]))
result["paired_on_minus_off"]["per_kernel_ms"] = {k: [float(dm[i]), float(dse[i])] for i, k in enumerate(names)}
print("paired on - off per kernel (ms, standard error): " + "  ".join("%s %+.4f (%.4f)" % (k, dm[i], dse[i]) for i, k in enumerate(names) if k not in ("clear", "frame")), flush=True)
print("paired on - off: stage 0 %+.4f ms (standard error %.4f)  resolve %+.4f ms (%.4f)  frame %+.4f ms (%.4f)" % (dm[2], dse[2], dm[6], dse[6], dm[8], dse[8]), flush=True)
for label in ("off", "on"):
    r = ctx[label]
    r.timing_enable(False)
    r.walk_stats_enable(True)
    r.orbit(DX, 0.0)
    r.frame(WARMUP + FRAMES + 1)
    result[label]["resolve_walk"] = r.walk_stats()["resolve"]
    if label == "on":
        result["stats"] = r.temporal_unbiased_stats()
    r.walk_stats_enable(False)
st = result["stats"]
print("shaded pixels %d, histories with Mk > 0 %.4f, kept out of Z %.4f, rays from a history's origin %.4f" % (
    st["merged"], st["valid"] / max(st["merged"], 1), st["excluded"] / max(st["merged"], 1), st["history_rays"] / max(st["merged"], 1)))
print("resolve walks: toggle off %d, toggle on %d" % (result["off"]["resolve_walk"]["walked"], result["on"]["resolve_walk"]["walked"]))
print("on / off: stage 0 %.3fx, resolve %.3fx, frame %.3fx" % (result["on"]["stage0_ms"] / result["off"]["stage0_ms"],
                                                              result["on"]["resolve_ms"] / result["off"]["resolve_ms"], result["on"]["frame_ms"] / result["off"]["frame_ms"]))
for c in ctx.values():
    c.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
