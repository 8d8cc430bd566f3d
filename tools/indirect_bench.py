"""GPU. What rt_indirect costs on the bench stand-in: three contexts in one process with the toggle at 0, 1 and 5 bounces, their frames
alternating, each timed with HIP events (rt_timing: the kernels back to back on one stream, no look-ahead); reports the means and the
per-frame paired difference against the toggle-off context with its standard error. Then the pass alone (rt_indirect_timing) at
every bounce count 1 .. 5, with the rays and the paths alive when each bounce starts (rt_indirect_stats), and the
yardstick measured side by side: rt_path_trace(8) (08_nee: the same paths plus a primary ray and a first-hit light sample) at
max_depth 2 and 6, wall clock over a run of launches, in both of its forms.
  python tools/indirect_bench.py [WxH] [--json FILE]"""
import json
import os
import sys
import time

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
args = sys.argv[1:]
W, H = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
WARMUP, FRAMES, PASS_FRAMES, PT_RUNS = 8, 64, 12, 20
tris = scenes.make_blocks_restir()


def renderer(bounces=0, **opt):
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options(**opt))
    r.indirect(bounces)
    r.timing_enable(True)
    return r


result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES)
ctx = {b: renderer(b) for b in (0, 1, 5)}
result["build_id"] = ctx[0].build_id()
rows = {b: [] for b in ctx}
order = list(ctx)
for f in range(1, WARMUP + FRAMES + 1):
    for b in order[f % 3:] + order[:f % 3]:  # who goes first rotates
        ctx[b].frame(f)
        t = ctx[b].timing()
        if f > WARMUP:
            rows[b].append((t["frame"], ctx[b].indirect_timing() if b else 0.0))
base = np.array(rows[0])[:, 0]
for b in ctx:
    a = np.array(rows[b])
    d = a[:, 0] - base
    result[f"frame_bounces_{b}"] = dict(frame_ms=float(a[:, 0].mean()), frame_sd=float(a[:, 0].std(ddof=1)), pass_ms=float(a[:, 1].mean()),
                                        paired_minus_off_ms=float(d.mean()), paired_se=float(d.std(ddof=1) / np.sqrt(len(d))))
    print("rt_indirect %d: frame %.4f ms (sd %.4f)  pass %.4f ms  paired against off %+.4f ms (standard error %.4f)"
          % (b, a[:, 0].mean(), a[:, 0].std(ddof=1), a[:, 1].mean(), d.mean(), d.std(ddof=1) / np.sqrt(len(d))), flush=True)
for b in (1, 5):
    ctx[b].close()

# the pass alone behind a frame of the toggle-off context, bounces 1 .. 5
r = ctx[0]
result["pass"] = {}
for b in range(1, 6):
    ms = []
    for k in range(PASS_FRAMES):
        r.indirect_pass(1000 + k, b)
        ms.append(r.indirect_timing())
    st = r.indirect_stats()
    ms = np.array(ms[2:])
    result["pass"][f"bounces_{b}"] = dict(ms=float(ms.mean()), sd=float(ms.std(ddof=1)), **st)
    print("pass bounces %d: %.4f ms (sd %.4f)  paths %d  rays %d  alive at the last bounce %d"
          % (b, ms.mean(), ms.std(ddof=1), st["paths"], st["rays"], st["alive_last"]), flush=True)

# the yardstick: 08_nee itself, wall clock over PT_RUNS launches
r.timing_enable(False)
result["path_trace_08"] = {}
for md in (2, 6):
    r.set_options(bench_options(max_depth=md))
    for name, wf in (("one_launch", 0), ("wavefront", 1)):
        r.tuning(api.Tune.PT_WAVEFRONT, wf)
        for k in range(3):
            r.path_trace(8, k + 1)
        r.sync()
        t0 = time.perf_counter()
        for k in range(PT_RUNS):
            r.path_trace(8, 10 + k)
        r.sync()
        ms = (time.perf_counter() - t0) * 1e3 / PT_RUNS
        result["path_trace_08"][f"{name}_depth_{md}"] = dict(ms=ms, rays=r.path_trace_rays())
        print("rt_path_trace(8) %-10s max_depth %d: %.4f ms  rays %d" % (name, md, ms, r.path_trace_rays()), flush=True)
r.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
