"""GPU. Ambient occlusion at 1920x1080 on blocks_ao.obj (same scene, size, camera (8,8,8) -> (0,0,0)
and 64 rays per hit pixel) through rt_path_trace(ctx, 6, 0), both layouts of RT_TUNE_AO_LAYOUT (rt_tuning key 27) alternated in ONE process.

Every repeat times, for each layout in turn, `--launches` launches after one warm-up (host clock around rt_sync; the launches
are back to back on the context's stream). Reported per layout: median / min / max ms per launch over the repeats, Gray/s in
the reference's rays (rt_path_trace_rays: W*H primary rays + 64 per hit pixel), and whether the image is the same for both.
Writes profiles/r07_ao_layouts.json (--out-dir: elsewhere).

--rocprof: afterwards, in a SEPARATE child process, the same launches under `rocprofv3 --kernel-trace --stats` (nothing else
traced); the per-kernel stats land in profiles/r07_ao_kernel_stats.json (the raw output goes to a temporary directory).

  python tools/ao_bench.py [--reps 7] [--launches 20] [--rocprof]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 1920, 1080
EYE, AT = (8.0, 8.0, 8.0), (0.0, 0.0, 0.0)
OBJ = os.path.join(ROOT, "tests", "golden", "assets", "blocks_ao.obj")
REF_MS = 30.3  # 06_ao_hiprt, blocks_ao.obj, 1920x1080 (the reference's GPU, with HIPRT)


def make_renderer():
    from cedec_2024_rt_amd import api, scenes

    r = api.Renderer(W, H)
    r.set_scene(scenes.load_obj(OBJ))
    r.lookat(EYE, AT)
    return r


def timed(r, layout, launches):
    from cedec_2024_rt_amd.types import Tune

    r.tuning(Tune.AO_LAYOUT, layout)
    r.path_trace(6, 0)  # warm-up
    r.sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        r.path_trace(6, 0)
    r.sync()
    return (time.perf_counter() - t0) * 1e3 / launches


def measure(reps, launches):
    from cedec_2024_rt_amd import api

    r = make_renderer()
    ms = {0: [], 1: []}
    images = {}
    for rep in range(reps):
        for layout in ((0, 1) if rep % 2 == 0 else (1, 0)):  # alternate which layout goes first
            ms[layout].append(timed(r, layout, launches))
            images[layout] = r.download(api.RT_BUF_PIXELS).tobytes()
    rays = r.path_trace_rays()
    out = {
        "what": "rt_path_trace(ctx, 6, 0): ambient occlusion (examples/06_ao_hiprt/06_ao_hiprt.cu:35-91), blocks_ao.obj, 1920x1080, "
                "camera (8,8,8) -> (0,0,0), fovy pi/4; ms per launch, host clock around rt_sync over back-to-back launches",
        "reps": reps, "launches_per_rep": launches, "rays_per_launch": rays,
        "same_image_both_layouts": images[0] == images[1],
        "reference_ms": REF_MS, "build_id": r.build_id(),
        "layouts": {},
    }
    for layout, name in ((0, "pixel_major"), (1, "ray_major")):
        v = ms[layout]
        med = statistics.median(v)
        out["layouts"][name] = {
            "rt_tuning_27": layout, "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
            "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2), "ms_all": [round(x, 4) for x in v],
            "gray_per_s": round(rays / med / 1e6, 3),
        }
    r.close()
    d = make_renderer()
    out["default_layout"] = d.tuning_get(api.Tune.AO_LAYOUT)
    d.close()
    return out


def rocprof(launches):
    """the launches under rocprofv3 --kernel-trace --stats, in a child process of their own"""
    outdir = tempfile.mkdtemp(prefix="ao_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "ao", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--launches", str(launches)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"rocprofv3 exited {p.returncode}: {p.stderr[-2000:]}")
    stats = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        raise SystemExit(f"no kernel_stats.csv under {outdir}")
    rows = list(csv.DictReader(open(stats[0])))
    shutil.rmtree(outdir, ignore_errors=True)
    return {"command": "rocprofv3 --kernel-trace --stats -- python tools/ao_bench.py --child --launches %d (layout 0 then 1, one warm-up each)" % launches,
            "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        r = make_renderer()
        for layout in (0, 1):
            timed(r, layout, a.launches)
        r.close()
        return
    res = measure(a.reps, a.launches)
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(a.out_dir, "r07_ao_layouts.json"), "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "what"}, indent=1))
    if a.rocprof:
        st = rocprof(a.launches)
        json.dump(st, open(os.path.join(a.out_dir, "r07_ao_kernel_stats.json"), "w"), indent=1)
        for row in st["kernels"]:
            if "k_ao" in row.get("Name", ""):
                print(row)


if __name__ == "__main__":
    main()
