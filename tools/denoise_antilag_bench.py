"""GPU. What rt_denoise_temporal_antilag costs where geometry moves every frame: two contexts in one process over the bench stand-in,
the toggle off and on, both with rt_denoise_temporal_motion on (--no-follow: both off); before every frame from the second on both
get the same rt_scene_update, a span of --count non-emissive triangles (default 4 096, the window of that size the most pixels show)
moved up and down by --dy in turn (the setup of tools/denoise_motion_bench.py), then rt_frame and rt_denoise_temporal. The contexts
alternate, who goes first alternates too, and every call of one pairs with the same call of the other. Reports per stage of
rt_denoise_temporal_timing the means and the paired difference on - off with its standard error; for the stage the toggle changes,
the kernels one by one: k_denoise_temporal{,_motion} of the off context against k_denoise_antilag_gather (stage - k_denoise_antilag)
and k_denoise_antilag (rt_denoise_temporal_antilag_timing) of the on context, with the bytes each has to move (counted below from
the participating pixels of the last call: every record of a buffer once, 16 B each) and what share of the HBM peak of 8.0 TB/s
(MI355X; 6.29 TB/s measured for a float4 copy) that is. At 1920 x 1080 a buffer is 33 MB and several of them fit the 256 MB last-level
cache together, so the share is a nominal figure: how far the kernel is from the least time the memory system allows. And the share
of participating pixels whose lambda' > 0 in the last call. Not a parity run: the two images differ by construction.
  python tools/denoise_antilag_bench.py [WxH] [--count N] [--dy UNITS] [--radius R] [--no-follow] [--json FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cedec_2024_rt_amd import api, scenes  # noqa: E402
from cedec_2024_rt_amd.types import bench_options  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


def _flag(name):
    if name in sys.argv:
        sys.argv.remove(name)
        return True
    return False


def kernel_bytes(part, total, follow):
    """bytes each kernel has to move: participating pixels read their two guide records and the accumulation, the four previous
    buffers once each (the 2 x 2 taps of neighbours overlap), the guide hit under follow-motion, and write their records; the others
    read the guide word and the accumulation and write theirs"""
    rest = total - part
    temporal = part * (48 + 64 + 32 + (16 if follow else 0)) + rest * (32 + 32)
    gather = temporal + total * 16                    # + {e, l_h}
    antilag = part * (16 + 16 + 16 + 16 + 32) + rest * (16 + 16 + 16)  # {e, l_h}, the guide normal, colour, moments; colour and moments back
    return dict(temporal=temporal, gather=gather, antilag=antilag)


out_json = _opt("--json", None)
COUNT = int(_opt("--count", "4096"))
DY = float(_opt("--dy", "0.5"))
RADIUS = _opt("--radius", None)
FOLLOW = not _flag("--no-follow")
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
    r.denoise_temporal_motion(FOLLOW)
    state = r.denoise_temporal_antilag(on, **(dict(radius=int(RADIUS)) if RADIUS else {}))
    r.timing_enable(True)
    ctx[label] = r
params = {k: state[k] for k in ("radius", "gradient_lo", "gradient_hi", "floor")}
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
SHOWN = int(win[FIRST])
assert SHOWN > 0, "no window of %d triangles without an emitter is visible" % COUNT
print("moving triangles [%d, %d): %d of %d pixels show them (%.3f); anti-lag %s; follow-motion %s" %
      (FIRST, FIRST + COUNT, SHOWN, W * H, SHOWN / (W * H), params, FOLLOW), flush=True)
mask = np.zeros(len(tris), bool)
mask[FIRST:FIRST + COUNT] = True
cur = dict(off=tris, on=tris)
rows = dict(off=[], on=[])
antilag_ms, adapted = [], 0

for f in range(1, WARMUP + FRAMES + 1):
    for label in (("off", "on") if f % 2 else ("on", "off")):
        r = ctx[label]
        if f > 1:
            cur[label] = scenes.move_triangles(cur[label], mask, (0.0, DY if f % 2 == 0 else -DY, 0.0))
            r.update_scene(np.ascontiguousarray(cur[label][FIRST:FIRST + COUNT]), first=FIRST)
        r.frame(f)
        r.L.rt_denoise_temporal(r.h, None, None)
        r.sync()
        t = r.denoise_temporal_timing()
        if f > WARMUP:
            rows[label].append([t[k] for k in stages])
            if label == "on":
                antilag_ms.append(r.denoise_temporal_antilag_timing())
                adapted += int(r.denoise_temporal_antilag()["adapted"])
            else:
                assert not r.denoise_temporal_antilag()["adapted"]
assert adapted == FRAMES, "every timed call of the on context is an adapted call"
a_off, a_on, k_al = np.array(rows["off"]), np.array(rows["on"]), np.array(antilag_ms)
se = lambda x: float(x.std(ddof=1) / np.sqrt(len(x)))  # noqa: E731
result = dict(size=[W, H], warmup=WARMUP, frames=FRAMES, first=FIRST, count=COUNT, dy=DY, pixels_on_span=SHOWN, follow_motion=FOLLOW,
              antilag=params, build_id=ctx["on"].build_id(), adapted_calls=adapted)
for label, a in (("off", a_off), ("on", a_on)):
    result[label] = dict({k + "_ms": float(a[:, i].mean()) for i, k in enumerate(stages)}, **{k + "_sd": float(a[:, i].std(ddof=1)) for i, k in enumerate(stages)})
    print("toggle %-3s " % label + "  ".join("%s %.4f" % (k, a[:, i].mean()) for i, k in enumerate(stages)), flush=True)
d = a_on - a_off
result["paired_on_minus_off"] = {k + "_ms": [float(d[:, i].mean()), se(d[:, i])] for i, k in enumerate(stages)}
print("paired on - off (ms, standard error): " + "  ".join("%s %+.4f (%.4f)" % (k, d[:, i].mean(), se(d[:, i])) for i, k in enumerate(stages)), flush=True)
# the kernels of the stage the toggle changes
mom = ctx["on"].download(api.RT_BUF_DENOISE_HISTORY)
part = int((mom[:, 2] > 0).sum())
nbytes = kernel_bytes(part, W * H, FOLLOW)
k_temporal, k_gather = a_off[:, 1], a_on[:, 1] - k_al
kernels = {}
for name, ms, key in (("k_denoise_temporal_motion" if FOLLOW else "k_denoise_temporal", k_temporal, "temporal"),
                      ("k_denoise_antilag_gather", k_gather, "gather"), ("k_denoise_antilag", k_al, "antilag")):
    rate = nbytes[key] / (ms.mean() * 1e-3)
    kernels[name] = dict(ms=float(ms.mean()), se=se(ms), bytes=int(nbytes[key]), bytes_per_s=float(rate), share_of_hbm_peak=float(rate / HBM_PEAK))
    print("%-28s %.4f ms (standard error %.4f)  %6.1f MB  %.2f TB/s = %.3f of the HBM peak" % (name, ms.mean(), se(ms), nbytes[key] / 1e6, rate / 1e12, rate / HBM_PEAK), flush=True)
dk = (k_gather + k_al) - k_temporal
result.update(kernels=kernels, participating_pixels=part, gather_plus_antilag_minus_temporal_ms=[float(dk.mean()), se(dk)],
              response_share=float((mom[mom[:, 2] > 0, 3] > 0).mean()), mean_response=float(mom[mom[:, 2] > 0, 3].mean()))
print("gather + antilag - temporal: %+.4f ms (standard error %.4f); participating pixels %d of %d; lambda' > 0 on %.4f of them, mean lambda' %.4f" %
      (dk.mean(), se(dk), part, W * H, result["response_share"], result["mean_response"]), flush=True)
for c in ctx.values():
    c.close()
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
