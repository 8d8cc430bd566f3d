"""GPU. What rt_light_grid costs and gains on the bench stand-in (scenes.make_blocks_restir, 1920 x 1080 by default), beside uniform
selection and rt_light_sampling's power mode (the shape of tools/light_sampling_bench.py):

1. time: stage 0 (rt_timing's raycast + generate_candidate brackets) and the frame, HIP events, frames un-overlapped as in bench.py's
   per-kernel loop (rt_tuning 14 = 0, 17 = 0). Three contexts (uniform, power, grid) live side by side in one process and take turns,
   ROUNDS rounds of FRAMES frames each; reported: the mean of the rounds' means and the standard deviation across rounds.
2. build: the wall time of rt_scene_set with the grid off and on and the grid's own share (rt_light_grid_build_ms), and the wall time of
   an rt_scene_update of the stand-in's whole light span (tools/scene_update_bench.py's span) with the grid off and on, alternating.
3. error: RMSE over R, G, B of the lit pixels of a 1-frame and an 8-frame accumulation against the mode's own LONG-frame accumulation,
   with the benchmark options (temporal + spatial reuse, history warm) and with both reuses off (the candidates alone), mean and
   spread over TRIALS trials; the long images' means; and the 1-frame error at equal time, RMSE x sqrt(frame time / uniform's frame
   time, medians of the rounds) (the error of independent frames falls with the square root of their number: an estimate, stated as one).
  python tools/light_grid_bench.py [WxH] [--cells N] [--clusters B] [--json FILE]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cedec_2024_rt_amd import api, scenes  # noqa: E402
from cedec_2024_rt_amd.types import bench_options  # noqa: E402


def _opt(name, default=None):
    if name in sys.argv:
        v = sys.argv[sys.argv.index(name) + 1]
        del sys.argv[sys.argv.index(name):sys.argv.index(name) + 2]
        return v
    return default


out_json = _opt("--json")
CELLS, CLUSTERS = int(_opt("--cells", api.LIGHT_GRID_DEFAULT[0])), int(_opt("--clusters", api.LIGHT_GRID_DEFAULT[1]))
LONG = int(_opt("--long", 2048))
W, H = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1920x1080").split("x"))
WARMUP, ROUNDS, FRAMES = 16, 6, 40
TRIALS = 6
UPDATES = 12
MODES = ("uniform", "power", "grid")
tris = scenes.make_blocks_restir()


def renderer(mode, **optkw):
    r = api.Renderer(W, H)
    if mode == "grid":
        r.light_grid(CELLS, CLUSTERS)
    elif mode == "power":
        r.light_sampling("power")
    t0 = time.perf_counter()
    r.set_scene(tris)
    r.scene_set_ms = (time.perf_counter() - t0) * 1e3
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options(**optkw))
    return r


result = dict(size=[W, H], scene=dict(triangles=len(tris)), grid=[CELLS, CLUSTERS], warmup=WARMUP, rounds=ROUNDS, frames_per_round=FRAMES, build=api.build_id())

# ---- 1. time
configs = [(m, renderer(m)) for m in MODES]
result["scene"]["lights"] = configs[0][1].scene_info()["lights"]
result["grid_built"] = list(dict(configs)["grid"].light_grid())
frame_no = {}
for label, r in configs:
    r.tuning(14, 0)
    r.tuning(17, 0)
    r.timing_enable(True)
    for f in range(1, WARMUP + 1):
        r.frame(f)
    frame_no[label] = WARMUP
per_round = {label: [] for label, _ in configs}
for rnd in range(ROUNDS):
    order = configs if rnd % 2 == 0 else configs[::-1]
    for label, r in order:
        rows = []
        for _ in range(FRAMES):
            frame_no[label] += 1
            r.frame(frame_no[label])
            t = r.timing()
            rows.append((t["raycast"] + t["generate_candidate"], t["frame"]))
        per_round[label].append(np.mean(rows, axis=0))
result["time_ms"] = {}
for label, r in configs:
    a = np.array(per_round[label])
    result["time_ms"][label] = dict(stage0=float(a[:, 0].mean()), stage0_sd=float(a[:, 0].std(ddof=1)), frame=float(a[:, 1].mean()),
                                    frame_sd=float(a[:, 1].std(ddof=1)), stage0_median=float(np.median(a[:, 0])), frame_median=float(np.median(a[:, 1])), stage0_rounds=[float(v) for v in a[:, 0]], frame_rounds=[float(v) for v in a[:, 1]],
                                    stage0_one_launch=bool(r.stage0_one_launch()))
    print("%-8s stage 0 %.4f ms (sd %.4f, median %.4f)  frame %.4f ms (sd %.4f, median %.4f)"
          % (label, a[:, 0].mean(), a[:, 0].std(ddof=1), np.median(a[:, 0]), a[:, 1].mean(), a[:, 1].std(ddof=1), np.median(a[:, 1])), flush=True)
tm = result["time_ms"]
print("medians of the rounds, grid / uniform: stage 0 %.3fx, frame %.3fx; grid / power: stage 0 %.3fx, frame %.3fx"
      % (tm["grid"]["stage0_median"] / tm["uniform"]["stage0_median"], tm["grid"]["frame_median"] / tm["uniform"]["frame_median"],
         tm["grid"]["stage0_median"] / tm["power"]["stage0_median"], tm["grid"]["frame_median"] / tm["power"]["frame_median"]), flush=True)

# ---- 2. build
ctx = dict(configs)
lights = scenes.light_indices(tris)
first, count = int(lights.min()), int(lights.max()) + 1 - int(lights.min())
mask = np.zeros(len(tris), bool)
mask[first:first + count] = True
sets = {m: [ctx[m].scene_set_ms] for m in ("uniform", "grid")}
grid_share = [ctx["grid"].light_grid_build_ms()]
for _ in range(3):
    for m in ("uniform", "grid"):
        t0 = time.perf_counter()
        ctx[m].set_scene(tris)
        sets[m].append((time.perf_counter() - t0) * 1e3)
    grid_share.append(ctx["grid"].light_grid_build_ms())
upd = {m: [] for m in ("uniform", "grid")}
grid_upd = []
cur = {m: tris for m in upd}
for k in range(UPDATES + 2):
    for m in (("uniform", "grid") if k % 2 else ("grid", "uniform")):
        cur[m] = scenes.move_triangles(cur[m], mask, (0.0, 0.05 if k % 2 == 0 else -0.05, 0.0))
        s = np.ascontiguousarray(cur[m][first:first + count])
        t0 = time.perf_counter()
        ctx[m].update_scene(s, first=first)
        ms = (time.perf_counter() - t0) * 1e3
        if k >= 2:
            upd[m].append(ms)
            if m == "grid":
                grid_upd.append(ctx[m].light_grid_build_ms())
        ctx[m].frame(1000 + k)
result["build_ms"] = dict(scene_set={m: dict(first=v[0], later_mean=float(np.mean(v[1:])), later=v[1:]) for m, v in sets.items()},
                          grid_share_of_scene_set=grid_share, span=dict(first=first, count=count, lights=int(len(lights))),
                          scene_update={m: dict(mean=float(np.mean(v)), sd=float(np.std(v, ddof=1)), all=v) for m, v in upd.items()},
                          grid_share_of_scene_update=dict(mean=float(np.mean(grid_upd)), sd=float(np.std(grid_upd, ddof=1))))
b = result["build_ms"]
print("rt_scene_set: grid off %.1f ms, on %.1f ms (the tables' share %.2f ms); rt_scene_update of %d triangles: off %.2f ms (sd %.2f), on %.2f ms (sd %.2f), the tables' share %.2f ms"
      % (b["scene_set"]["uniform"]["later_mean"], b["scene_set"]["grid"]["later_mean"], float(np.mean(grid_share)), count, b["scene_update"]["uniform"]["mean"],
         b["scene_update"]["uniform"]["sd"], b["scene_update"]["grid"]["mean"], b["scene_update"]["grid"]["sd"], b["grid_share_of_scene_update"]["mean"]), flush=True)
for _, r in configs:
    r.close()


# ---- 3. error
def image(r):
    a = r.download(api.RT_BUF_ACCUMULATION).astype(np.float64)
    n = np.maximum(a[:, 3:4], 1.0)
    return a[:, :3] / n


result["rmse"] = {}
for setup, optkw in (("bench_options", dict()), ("candidates_only", dict(use_temporal_resampling=0, use_spatial_resampling=0))):
    long_img, short = {}, {}
    for mode in MODES:
        r = renderer(mode, accumulate=1, **optkw)
        f = 0
        for _ in range(8):  # history warm
            f += 1
            r.frame(f)
        short[mode] = {1: [], 8: []}
        for trial in range(TRIALS):
            for n in (1, 8):
                for k in range(n):
                    f += 1
                    r.frame(f, clear_first=(k == 0))
                short[mode][n].append(image(r))
        for k in range(LONG):
            f += 1
            r.frame(f, clear_first=(k == 0))
        long_img[mode] = image(r)
        r.close()
    lit = np.zeros(W * H, bool)
    for m in MODES:
        lit |= long_img[m].sum(axis=1) > 0
    e = dict(long_frames=LONG, trials=TRIALS, pixels=int(lit.sum()), mean_rgb_sum={m: float(long_img[m][lit].sum(axis=1).mean()) for m in MODES},
             long_vs_long_uniform={m: float(np.sqrt(((long_img[m] - long_img["uniform"])[lit] ** 2).mean())) for m in ("power", "grid")},
             median_abs_error_1_frame={m: float(np.median([np.median(np.abs(img - long_img[m])[lit]) for img in short[m][1]])) for m in MODES})
    for mode in MODES:
        for n in (1, 8):
            v = [float(np.sqrt(((img - long_img[mode])[lit] ** 2).mean())) for img in short[mode][n]]
            e["%s_%d_frame" % (mode, n)] = dict(mean=float(np.mean(v)), sd=float(np.std(v, ddof=1)), min=float(np.min(v)), max=float(np.max(v)), trials=v)
        e["%s_1_frame_at_equal_time" % mode] = e["%s_1_frame" % mode]["mean"] * float(np.sqrt(tm[mode]["frame_median"] / tm["uniform"]["frame_median"]))
    result["rmse"][setup] = e
    for n in (1, 8):
        print("%s: RMSE of %d frame(s) against the own long accumulation: " % (setup, n)
              + ", ".join("%s %.4f (sd %.4f, %.4f .. %.4f)" % (m, e["%s_%d_frame" % (m, n)]["mean"], e["%s_%d_frame" % (m, n)]["sd"], e["%s_%d_frame" % (m, n)]["min"],
                                                               e["%s_%d_frame" % (m, n)]["max"]) for m in MODES), flush=True)
    print("    at equal time (1 frame): " + ", ".join("%s %.4f" % (m, e["%s_1_frame_at_equal_time" % m]) for m in MODES)
          + "; mean R+G+B of the long images %s; long image against uniform's %s; median |error| of a 1-frame image %s"
          % (e["mean_rgb_sum"], e["long_vs_long_uniform"], e["median_abs_error_1_frame"]), flush=True)
if out_json:
    with open(out_json, "w") as fjson:
        json.dump(result, fjson, indent=1)
