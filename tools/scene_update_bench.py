"""GPU. Cost of rt_scene_update (the refit of csrc/bvh_refit.h) on the blocks_restir stand-in at 1920x1080, bench options.

Records, in profiles/r14_scene_update.json (--out-dir / --out-name: elsewhere; r08's run is profiles/r08_scene_update.json):
  * rt_scene_set: wall ms (rt_build_ms) of the first and of repeated calls;
  * rt_scene_update, each call synchronised (the call itself waits): the whole array, and the span from the lowest to the
    highest emissive index with every light moved (median / min / max over --reps calls; the first call of a scene also
    lists the tree's levels, so it is reported apart);
  * frame ms (host clock around rt_sync, --frames back-to-back rt_frames after a warm-up) right after a rebuild, after 60
    light-moving refits, and after one 4096-triangle span was moved by three scene extents: what the refitted tree costs
    the walks (reported, not gated); beside each of the two refitted states rt_bvh_cost's now / at_build, the figure a caller
    has for deciding on a rebuild, and the frame-time ratio to the rebuild of the same scene;
  * --rocprof: the refit kernels' device time from a SEPARATE child process under `rocprofv3 --kernel-trace --stats`
    (nothing else traced): --reps light-span updates.

  python tools/scene_update_bench.py [--reps 20] [--frames 30] [--rocprof]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 1920, 1080
REFIT_KERNELS = ("k_refit_level", "k_bvh_cost", "k_frag_", "k_refit_topo", "k_refit_topo_next", "k_refit_bounds", "k_light_table", "k_trimat", "k_bvh_tv")


def setup():
    from cedec_2024_rt_amd import api, scenes
    from cedec_2024_rt_amd.types import bench_options

    tris = scenes.make_blocks_restir()
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options())
    lights = scenes.light_indices(tris)
    lmask = np.zeros(len(tris), bool)
    lmask[lights] = True
    return r, tris, lmask, int(lights.min()), int(lights.max()) + 1


def stats(v):
    med = statistics.median(v)
    return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "ms_all": [round(x, 4) for x in v]}


def timed_update(r, span, first):
    t0 = time.perf_counter()
    r.update_scene(span, first)  # returns after the device work is done
    return (time.perf_counter() - t0) * 1e3


def frame_ms(r, frames, start):
    r.frame(start, clear_first=True)
    r.frame(start + 1)
    r.sync()
    t0 = time.perf_counter()
    for f in range(start + 2, start + 2 + frames):
        r.frame(f)
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / frames


def cost(r):
    """rt_bvh_cost after refits: what the tree costs now, what it cost as built, and the ratio a caller acts on"""
    now, at_build = r.bvh_cost()
    return {"now": round(now, 4), "at_build": round(at_build, 4), "ratio": round(now / at_build, 4)}


def measure(reps, frames):
    from cedec_2024_rt_amd import scenes

    r, tris, lmask, lo, hi = setup()
    out = {
        "what": "rt_scene_update on the blocks_restir stand-in (scenes.make_blocks_restir), %dx%d, bench options; wall ms of "
                "synchronised calls (host clock), frame ms = host clock around rt_sync over back-to-back rt_frames" % (W, H),
        "triangles": len(tris), "lights": int(lmask.sum()), "light_span": [lo, hi], "build_id": r.build_id(),
        "bvh_info": r.bvh_info(),
    }
    out["rt_scene_set_ms_first"] = round(r.build_ms(), 3)
    sets = []
    for _ in range(3):
        r.set_scene(tris)
        sets.append(r.build_ms())
    out["rt_scene_set_ms"] = stats(sets)
    base = frame_ms(r, frames, 1)
    out["frame_ms_after_rebuild"] = round(base, 4)
    cur = tris
    out["first_update_ms"] = round(timed_update(r, cur, 0), 3)  # lists the tree's levels, then refits
    whole = [timed_update(r, cur, 0) for _ in range(reps)]
    out["update_whole_array"] = stats(whole)
    light = []
    for _ in range(60):
        cur = scenes.move_triangles(cur, lmask, (0.01, 0.0, -0.01))
        light.append(timed_update(r, cur[lo:hi], lo))
    out["update_light_span"] = dict(stats(light), calls=len(light), triangles=hi - lo, bytes=(hi - lo) * 60)
    out["frame_ms_after_60_light_refits"] = round(frame_ms(r, frames, 1000), 4)
    out["bvh_cost_after_60_light_refits"] = cost(r)
    r.set_scene(cur)
    out["frame_ms_after_rebuild_of_the_same_scene"] = round(frame_ms(r, frames, 2000), 4)
    out["bvh_cost_after_rebuild_of_the_same_scene"] = cost(r)
    out["frame_ratio_60_light_refits_to_rebuild"] = round(out["frame_ms_after_60_light_refits"] / out["frame_ms_after_rebuild_of_the_same_scene"], 3)
    v = cur["v"].reshape(-1, 3)
    ext = float((v.max(0) - v.min(0)).max())
    a = len(cur) // 2
    blk = np.zeros(len(cur), bool)
    blk[a:a + 4096] = True
    far = scenes.move_triangles(cur, blk, (3.0 * ext, 0.0, 0.0))
    r.update_scene(far[a:a + 4096], a)
    out["frame_ms_after_far_block_refit"] = round(frame_ms(r, frames, 3000), 4)
    out["bvh_cost_after_far_block_refit"] = cost(r)
    r.set_scene(far)
    out["frame_ms_after_far_block_rebuild"] = round(frame_ms(r, frames, 4000), 4)
    out["bvh_cost_after_far_block_rebuild"] = cost(r)
    out["frame_ratio_far_block_refit_to_rebuild"] = round(out["frame_ms_after_far_block_refit"] / out["frame_ms_after_far_block_rebuild"], 3)
    out["far_block"] = {"first": a, "count": 4096, "offset_x": round(3.0 * ext, 3)}
    r.close()
    return out


def child(reps):
    from cedec_2024_rt_amd import scenes

    r, tris, lmask, lo, hi = setup()
    cur = tris
    r.update_scene(cur, 0)  # the level lists
    for _ in range(reps):
        cur = scenes.move_triangles(cur, lmask, (0.01, 0.0, -0.01))
        r.update_scene(cur[lo:hi], lo)
    r.close()


def rocprof(reps):
    outdir = tempfile.mkdtemp(prefix="refit_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "refit", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"rocprofv3 exited {p.returncode}: {p.stderr[-2000:]}")
    found = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit(f"no kernel_stats.csv under {outdir}")
    rows = [row for row in csv.DictReader(open(found[0])) if any(k in row.get("Name", "") for k in REFIT_KERNELS)]
    shutil.rmtree(outdir, ignore_errors=True)
    level = [row for row in rows if "k_refit_level" in row.get("Name", "")]
    total_ns = sum(float(row["TotalDurationNs"]) for row in level) if level else 0.0
    return {"command": "rocprofv3 --kernel-trace --stats -- python tools/scene_update_bench.py --child --reps %d "
                       "(one whole-array update, then %d light-span updates)" % (reps, reps),
            "k_refit_level_device_ms_per_update": round(total_ns / 1e6 / (reps + 1), 4), "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--out-name", default="r14_scene_update.json")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.reps)
        return
    res = measure(a.reps, a.frames)
    if a.rocprof:
        res["refit_kernels"] = rocprof(a.reps)
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(a.out_dir, a.out_name), "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("what",)}, indent=1)[:6000])


if __name__ == "__main__":
    main()
