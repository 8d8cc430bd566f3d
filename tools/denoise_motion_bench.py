"""GPU. What rt_denoise_temporal_motion costs and keeps where geometry moves every frame: two contexts in one process over the bench
stand-in, the toggle off and on; before every frame from the second on both get the same rt_scene_update, a span of non-emissive
triangles moved up and down by --dy in turn (the setup of tools/temporal_motion_bench.py), then rt_frame and rt_denoise_temporal. The
span is the window of triangles without an emitter that the most pixels of the first frame show: --count triangles, or by default the
smallest power of two at which about a quarter of the pixels show it. The contexts alternate, who goes first alternates too, and every
call of one pairs with the same call of the other. Reports per stage of rt_denoise_temporal_timing the means and the paired difference
on - off, the rt_scene_update wall time likewise, and from RT_BUF_DENOISE_HISTORY of the last call the share of the span's
participating pixels that keep h > 1 and that reached h >= 4 (where the variance comes from the history). Not a parity run: the two
images differ by construction.
  python tools/denoise_motion_bench.py [WxH] [--count N] [--dy UNITS] [--json FILE]"""
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
COUNT = int(_opt("--count", "0"))
DY = float(_opt("--dy", "0.5"))
args = sys.argv[1:]
W, H = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
WARMUP, FRAMES = 8, 96
tris = scenes.make_blocks_restir()
stages = ("guide", "reprojection", "variance", "levels", "last_level", "total")
ctx = {}
for label, on in (("off", False), ("on", True)):
    r = api.Renderer(W, H)
    r.set_scene(tris)
    r.lookat(scenes.BLOCKS_RESTIR_EYE, scenes.BLOCKS_RESTIR_LOOKAT)
    r.set_options(bench_options(accumulate=0))
    r.denoise_temporal_motion(on)
    r.timing_enable(True)
    ctx[label] = r
# the span: pixels per triangle of the first frame's primary rays, summed over windows of COUNT triangles without an emitter
r = ctx["off"]
r.raycast()
idx = r.download(api.RT_BUF_VISIBILITY)["index"]
seen = np.bincount(idx[idx >= 0], minlength=len(tris)).astype(np.int64)
emissive = (tris["emissive"] > 0).any(axis=1).astype(np.int64)
c_seen, c_emi = np.concatenate([[0], np.cumsum(seen)]), np.concatenate([[0], np.cumsum(emissive)])


def best_window(count):
    win = c_seen[count:] - c_seen[:-count]
    win[(c_emi[count:] - c_emi[:-count]) > 0] = -1
    first = int(np.argmax(win))
    return first, int(win[first])


if COUNT:
    COUNT = min(COUNT, len(tris))
    FIRST, SHOWN = best_window(COUNT)
else:
    COUNT = 256
    FIRST, SHOWN = best_window(COUNT)
    while 4 * SHOWN < W * H and 2 * COUNT <= len(tris):
        COUNT *= 2
        FIRST, SHOWN = best_window(COUNT)
assert SHOWN > 0, "no window of %d triangles without an emitter is visible" % COUNT
print("moving triangles [%d, %d): %d of %d pixels show them (%.3f)" % (FIRST, FIRST + COUNT, SHOWN, W * H, SHOWN / (W * H)), flush=True)
mask = np.zeros(len(tris), bool)
mask[FIRST:FIRST + COUNT] = True
cur = dict(off=tris, on=tris)
rows = dict(off=[], on=[])
upd = dict(off=[], on=[])
followed = dict(off=0, on=0)


def step(label, f):
    r = ctx[label]
    if f > 1:
        cur[label] = scenes.move_triangles(cur[label], mask, (0.0, DY if f % 2 == 0 else -DY, 0.0))
        span = np.ascontiguousarray(cur[label][FIRST:FIRST + COUNT])
        t0 = time.perf_counter()
        r.update_scene(span, first=FIRST)
        if f > WARMUP:
            upd[label].append((time.perf_counter() - t0) * 1e3)
    r.frame(f)
    r.L.rt_denoise_temporal(r.h, None, None)
    r.sync()
    if f > WARMUP:
        followed[label] += int(r.denoise_temporal_motion()["followed"])


for f in range(1, WARMUP + FRAMES + 1):
    for label in (("off", "on") if f % 2 else ("on", "off")):
        step(label, f)
        t = ctx[label].denoise_temporal_timing()
        if f > WARMUP:
            rows[label].append([t[k] for k in stages])
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES, first=FIRST, count=COUNT, dy=DY, pixels_on_span=SHOWN, span_share=SHOWN / (W * H),
              build_id=ctx["on"].build_id(), followed_calls=followed)
for label in ("off", "on"):
    a, u = np.array(rows[label]), np.array(upd[label])
    m, sd = a.mean(axis=0), a.std(axis=0, ddof=1)
    result[label] = dict({k + "_ms": float(m[i]) for i, k in enumerate(stages)}, **{k + "_sd": float(sd[i]) for i, k in enumerate(stages)},
                         scene_update_ms=float(u.mean()), scene_update_sd=float(u.std(ddof=1)))
    print("toggle %-3s " % label + "  ".join("%s %.4f" % (k, m[i]) for i, k in enumerate(stages)) +
          "  rt_scene_update %.4f ms (sd %.4f, host clock); followed calls %d of %d" % (u.mean(), u.std(ddof=1), followed[label], FRAMES), flush=True)
d = np.array(rows["on"]) - np.array(rows["off"])
dmean, dse = d.mean(axis=0), d.std(axis=0, ddof=1) / np.sqrt(len(d))
du = np.array(upd["on"]) - np.array(upd["off"])
result["paired_on_minus_off"] = dict({k + "_ms": [float(dmean[i]), float(dse[i])] for i, k in enumerate(stages)},
                                     scene_update_ms=[float(du.mean()), float(du.std(ddof=1) / np.sqrt(len(du)))])
print("paired on - off (ms, standard error): " + "  ".join("%s %+.4f (%.4f)" % (k, dmean[i], dse[i]) for i, k in enumerate(stages)) +
      "  rt_scene_update %+.4f (%.4f)" % (du.mean(), du.std(ddof=1) / np.sqrt(len(du))), flush=True)
# the history the last call left: the span's participating pixels (h > 0) of each context
for label in ("off", "on"):
    r = ctx[label]
    h = r.download(api.RT_BUF_DENOISE_HISTORY)[:, 2]
    word = r.download(api.RT_BUF_DENOISE_GUIDE).view(np.int32).reshape(-1, 4)[:, 2]
    on_span = (word >= FIRST) & (word < FIRST + COUNT) & (h > 0)
    n = max(int(on_span.sum()), 1)
    result[label].update(span_pixels=int(on_span.sum()), keep_share=float((h[on_span] > 1).sum() / n), variance_from_history_share=float((h[on_span] >= 4).sum() / n),
                         mean_h=float(h[on_span].mean()) if on_span.any() else 0.0)
    print("toggle %-3s participating pixels on the span %d: h > 1 on %.4f, h >= 4 on %.4f, mean h %.2f" %
          (label, on_span.sum(), result[label]["keep_share"], result[label]["variance_from_history_share"], result[label]["mean_h"]), flush=True)
for c in ctx.values():
    c.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
