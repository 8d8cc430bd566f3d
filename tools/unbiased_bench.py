"""GPU. What rt_spatial_unbiased costs: the spatial passes and the frame timed (HIP events, rt_timing) on the bench stand-in with the mode
on, against the reference's (biased) frame of the same process, and the shadow rays the pass walks per shaded pixel and pass
(rt_walk_stats). Not a parity run: the two images differ by construction.
  python tools/unbiased_bench.py [WxH] [--json FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cedec_2024_rt_amd import api, scenes  # noqa: E402
from cedec_2024_rt_amd.types import bench_options  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--json"]
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if out_json:
    args.remove(out_json)
W, H = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
WARMUP, FRAMES = 8, 32
tris = scenes.make_blocks_restir()
names = ("clear", "raycast", "generate_candidate", "spatial0", "spatial1", "spatial2", "resolve", "tone_mapping", "frame")
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES)
for label, on in (("biased", False), ("unbiased", True)):
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options())
    r.spatial_unbiased(on)
    r.timing_enable(True)
    rows = []
    for f in range(1, WARMUP + FRAMES + 1):
        r.frame(f)
        t = r.timing()
        if f > WARMUP:
            rows.append([t[k] for k in names])
    rows = np.array(rows)
    m, sd = rows.mean(axis=0), rows.std(axis=0, ddof=1)
    r.timing_enable(False)
    # one more frame with the walk counters (such a frame traces its primary rays and is not timed)
    r.walk_stats_enable(True)
    r.frame(WARMUP + FRAMES + 1)
    r.sync()
    ws = r.walk_stats()["spatial_resampling"]
    r.walk_stats_enable(False)
    shaded = int(r.ray_count()[1])
    per = 3.0 * max(shaded, 1)
    result[label] = dict(spatial_ms=[float(v) for v in m[3:6]], spatial_sd=[float(v) for v in sd[3:6]], resolve_ms=float(m[6]), frame_ms=float(m[8]),
                         frame_sd=float(sd[8]), shaded_pixels=shaded, rays_walked_per_pixel_and_pass=ws["walked"] / per,
                         rays_self_test_per_pixel_and_pass=ws["self_test"] / per, own_rays_known_per_pixel_and_pass=ws["not_evaluated"] / per)
    print("%-9s spatial %.4f + %.4f + %.4f ms (sd %.4f %.4f %.4f)  resolve %.4f  frame %.4f ms (sd %.4f)  walked %.3f rays per shaded pixel and pass "
          "(+ %.3f settled by the origin's triangle, %.3f own rays known)" % (label, m[3], m[4], m[5], sd[3], sd[4], sd[5], m[6], m[8], sd[8],
                                                                             ws["walked"] / per, ws["self_test"] / per, ws["not_evaluated"] / per), flush=True)
    r.close()
print("unbiased / biased: spatial passes %.2fx, frame %.2fx" % (sum(result["unbiased"]["spatial_ms"]) / sum(result["biased"]["spatial_ms"]),
                                                               result["unbiased"]["frame_ms"] / result["biased"]["frame_ms"]))
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
