#!/usr/bin/env python3
"""rt_denoise device time (HIP events inside the call, rt_denoise_timing) on the bench stand-in: per kernel group (guide, prep =
demodulation + variance, the levels before the last, the last level with the fused output), for 1 to 8 iterations and both layouts
of rt_tuning key 28 (0 per-lane gathers, 1 residue lattice in LDS), default parameters otherwise. Also the frame's own raycast launch
(rt_timing with rt_tuning 25 = 0) for comparison with the guide pass. Medians of --reps calls after --warmup calls.

  python tools/denoise_bench.py [--width 1920 --height 1080] [--reps 20] [--out profiles/r09_denoise.json]

--temporal: rt_denoise_temporal instead (rt_denoise_temporal_timing: guide, reprojection + integration, variance, the levels before
the last, the last level, whole call) in steady state: a ReSTIR frame (accumulate = 0) and one call per frame under an orbit of
--orbit-dx px per frame; medians over --reps calls after the first --warmup-calls (>= 8), for 0, 1, 5 and 8 iterations and both
layouts; rt_denoise on the same frames for comparison.

  python tools/denoise_bench.py --temporal [--reps 20] [--out profiles/r10_denoise_temporal.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--temporal", action="store_true")
    ap.add_argument("--warmup-calls", type=int, default=10)
    ap.add_argument("--orbit-dx", type=float, default=12.0)
    a = ap.parse_args()
    if a.temporal:
        return temporal(a)
    from cedec_2024_rt_amd import api, scenes
    from cedec_2024_rt_amd.types import bench_options

    W, H = a.width, a.height
    r = api.Renderer(W, H)
    r.set_scene(scenes.make_blocks_restir())
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options(accumulate=1))
    r.tuning(api.Tune.FUSE_RAYCAST, 0)  # the frame's raycast as a launch of its own (timed as ms[1])
    r.tuning(api.Tune.SPEC, 0)
    r.timing_enable(True)
    raycast = []
    for f in range(1, 4 + a.reps):
        r.frame(f)
        r.sync()
        if f > 3:
            raycast.append(r.timing()["raycast"])
    out = dict(tool="tools/denoise_bench.py", build_id=api.build_id(), size=[W, H], scene="scenes.make_blocks_restir (bench stand-in)",
               reps=a.reps, unit="ms (median, HIP events on the context's stream)", raycast_ms=float(np.median(raycast)), layouts={})
    for lay in (0, 1):
        r.tuning(api.Tune.DN_LAYOUT, lay)
        rows = {}
        for it in range(1, 9):
            for _ in range(a.warmup):
                r.denoise(iterations=it)
            t = []
            for _ in range(a.reps):
                r.denoise(iterations=it)
                t.append(r.denoise_timing())
            med = {k: float(np.median([x[k] for x in t])) for k in t[0]}
            med["filter"] = med["prep"] + med["levels"] + med["last_level"]
            rows[str(it)] = med
            print(f"layout {lay} iterations {it}: " + ", ".join(f"{k} {v:.4f}" for k, v in med.items()), flush=True)
        out["layouts"][str(lay)] = rows
    r.close()
    print(json.dumps(dict(raycast_ms=out["raycast_ms"])))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def temporal(a):
    from cedec_2024_rt_amd import api, scenes
    from cedec_2024_rt_amd.types import bench_options

    if a.warmup_calls < 8:
        raise SystemExit("--warmup-calls: at least 8 (steady state: the history caps its variance window at h >= 4)")
    W, H = a.width, a.height
    r = api.Renderer(W, H)
    r.set_scene(scenes.make_blocks_restir())
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options(accumulate=0))
    r.timing_enable(True)
    out = dict(tool="tools/denoise_bench.py --temporal", build_id=api.build_id(), size=[W, H], scene="scenes.make_blocks_restir (bench stand-in)",
               frames="rt_frame (accumulate = 0), rt_camera_orbit(%g, 0) before each" % a.orbit_dx, warmup_calls=a.warmup_calls, reps=a.reps,
               unit="ms (median, HIP events on the context's stream)", layouts={})
    frame = 0
    for lay in (0, 1):
        r.tuning(api.Tune.DN_LAYOUT, lay)
        rows = {}
        for it in (0, 1, 5, 8):
            r.denoise_temporal_reset()
            t, s, h4 = [], [], []
            for k in range(a.warmup_calls + a.reps):
                frame += 1
                r.orbit(a.orbit_dx, 0.0)
                r.frame(frame)
                r.denoise_temporal(iterations=it)
                if k >= a.warmup_calls:
                    t.append(r.denoise_temporal_timing())
                    hist = r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2]
                    h4.append(float(np.mean(hist[hist > 0] >= 4)))
                    r.denoise(iterations=it)
                    s.append(r.denoise_timing()["total"])
            med = {k: float(np.median([x[k] for x in t])) for k in t[0]}
            med["rt_denoise_total"] = float(np.median(s))
            med["history_ge4_fraction"] = float(np.median(h4))
            rows[str(it)] = med
            print(f"layout {lay} iterations {it}: " + ", ".join(f"{k} {v:.4f}" for k, v in med.items()), flush=True)
        out["layouts"][str(lay)] = rows
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
