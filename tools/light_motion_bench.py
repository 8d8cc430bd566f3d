"""GPU. What rt_temporal_light_motion costs where lights move every frame: two contexts in one process over the bench stand-in, one with
the toggle off and one with it on, the same scenes in both, paired per update (after the pattern of tools/temporal_motion_bench.py).

  python tools/light_motion_bench.py [WxH] [--json profiles/r32_light_motion.json] [--frames 48] [--parent-lib PATH]

--parent-lib: a build of the parent commit's library; a third context runs it beside the two, the same scenes and the same
alternation, so that rt_scene_update with the toggle off is held against the parent's in the same process.

Two spans: the whole light span of the stand-in (the span of tools/scene_update_bench.py) and a small lamp, the first two emissive
triangles. For each: wall ms of rt_scene_update per context (host clock; the call returns after the device work), the paired difference
on - off, the device ms of the re-basing launches alone (rt_temporal_light_motion_timing), the share of records located and moved, and
for the small span both locate paths (rt_temporal_light_motion_path): the direct loop and the point query on the old tree."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
FRAMES = int(_opt("--frames", "48"))
PARENT = _opt("--parent-lib", None)
WARMUP = 6
args = sys.argv[1:]
W, H = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
tris = scenes.make_blocks_restir()
lights = scenes.light_indices(tris)
SPANS = {"all lights": (int(lights.min()), int(lights.max()) + 1 - int(lights.min())), "small lamp": (int(lights[0]), 2)}
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES, triangles=len(tris), lights=len(lights))


def context(on, lib_path=None):
    r = api.Renderer(W, H, lib_path=lib_path)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options())
    if lib_path is None:
        r.temporal_light_motion(on)
    r.timing_enable(True)
    return r


def run(span, path):
    first, count = SPANS[span]
    n_lights = int(((lights >= first) & (lights < first + count)).sum())
    mask = np.zeros(len(tris), bool)
    mask[first:first + count] = True
    ctx = dict(off=context(False), on=context(True))
    ctx["on"].temporal_light_motion_path(path)
    if PARENT:
        ctx["parent"] = context(False, PARENT)
    cur = {k: tris for k in ctx}
    upd, dev = {k: [] for k in ctx}, []
    order = list(ctx)
    for f in range(1, WARMUP + FRAMES + 1):
        for label in (order if f % 2 else order[::-1]):  # who goes first alternates too
            r = ctx[label]
            if f > 1:
                cur[label] = scenes.move_triangles(cur[label], mask, (0.0, 0.05 if f % 2 == 0 else -0.05, 0.0))
                s = np.ascontiguousarray(cur[label][first:first + count])
                t0 = time.perf_counter()
                r.update_scene(s, first=first)
                ms = (time.perf_counter() - t0) * 1e3
                if f > WARMUP:
                    upd[label].append(ms)
                    if label == "on":
                        dev.append(r.temporal_light_motion_timing())
            r.frame(f)
    st = ctx["on"].temporal_light_motion_stats()
    on_, off_ = np.array(upd["on"]), np.array(upd["off"])
    d = on_ - off_
    row = dict(first=first, count=count, span_lights=n_lights, path="direct loop" if n_lights <= path else "point query",
               update_off_ms=float(off_.mean()), update_off_sd=float(off_.std(ddof=1)), update_on_ms=float(on_.mean()), update_on_sd=float(on_.std(ddof=1)),
               paired_on_minus_off_ms=float(d.mean()), paired_se=float(d.std(ddof=1) / np.sqrt(len(d))),
               rebase_device_ms=float(np.mean(dev)), rebase_device_sd=float(np.std(dev, ddof=1)), buffers_per_update=st["buffers"] / (WARMUP + FRAMES - 1),
               located_share=st["located"] / max(st["examined"], 1), moved_share=st["moved"] / max(st["examined"], 1), stats=st)
    if PARENT:
        p_ = np.array(upd["parent"])
        dp = off_ - p_
        row.update(update_parent_ms=float(p_.mean()), update_parent_sd=float(p_.std(ddof=1)), paired_off_minus_parent_ms=float(dp.mean()),
                   paired_off_minus_parent_se=float(dp.std(ddof=1) / np.sqrt(len(dp))))
        print("%-10s parent's rt_scene_update %.4f ms (sd %.4f)  paired toggle off - parent %+.4f ms (standard error %.4f)" %
              (span, row["update_parent_ms"], row["update_parent_sd"], row["paired_off_minus_parent_ms"], row["paired_off_minus_parent_se"]), flush=True)
    print("%-10s %-11s rt_scene_update off %.4f ms (sd %.4f)  on %.4f ms (sd %.4f)  paired on - off %+.4f ms (standard error %.4f)  re-basing launches %.4f ms "
          "(%.1f buffers)  located %.4f, moved %.4f of the examined records" %
          (span, row["path"], row["update_off_ms"], row["update_off_sd"], row["update_on_ms"], row["update_on_sd"], row["paired_on_minus_off_ms"], row["paired_se"],
           row["rebase_device_ms"], row["buffers_per_update"], row["located_share"], row["moved_share"]), flush=True)
    for c in ctx.values():
        c.close()
    return row


_r = api.Renderer(8, 8)
result["build_id"] = _r.build_id()
_r.close()
result["runs"] = [run("all lights", 0), run("small lamp", 1 << 30), run("small lamp", 0)]
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
