"""CPU. The grid rt_denoise_temporal_antilag's defaults come from (docs/MEASUREMENT_LOG_r30.md): radius x (gradient_lo, gradient_hi) x
floor through the two studies of tests/test_denoise_antilag_cpu.py, the moving box (relative MSE over `rest`, the pixels not on the
box, and over the box with follow-motion on; still camera and orbit) and the static scene (ratio to raw, orbit and still camera).
The choice: the lowest rest error (mean of still and orbit) among the points whose static-orbit ratio stays below spatial-only's.

  python tools/denoise_antilag_grid.py [--offsets 24] [--json out.json]"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RADII, RAMPS, FLOORS = (2, 3, 4), ((0.2, 0.8), (0.3, 1.0)), (0.02, 0.05, 0.1, 0.2, 0.4)


def main():
    import test_denoise_antilag_cpu as t
    from oracle import binding as ob

    ob.lib()
    ob.set_threads(ob.effective_cpus())
    offsets = int(sys.argv[sys.argv.index("--offsets") + 1]) if "--offsets" in sys.argv else t.STUDY_OFFSETS
    worlds = t.Worlds(ob)
    points = {f"r{r}_lo{lo}_hi{hi}_f{fl}": dict(radius=r, gradient_lo=lo, gradient_hi=hi, floor=fl) for r, (lo, hi), fl in itertools.product(RADII, RAMPS, FLOORS)}
    rows = {k: dict(al) for k, al in points.items()}
    base = {}
    for mode in ("still", "orbit"):
        cfg = {k: dict(antilag=True, al=al) for k, al in points.items()}
        cfg.update({"F" + k: dict(on=True, antilag=True, al=al) for k, al in points.items()})
        cfg.update(off=dict(), follow_off=dict(on=True))
        r = t.moving_box_study(ob, worlds, mode, cfg, offsets=offsets)
        for k in points:
            rows[k]["rest_" + mode] = float(r[k]["rest"].mean())
            rows[k]["box_follow_" + mode] = float(r["F" + k]["box"].mean())
        for k in ("raw", "spatial", "off", "follow_off"):
            base[f"{k}_{mode}"] = dict(rest=float(r[k]["rest"].mean()), box=float(r[k]["box"].mean()))
    for still in (False, True):
        name = "still" if still else "orbit"
        r = t.static_study(ob, still, points)
        for k in points:
            rows[k]["static_" + name] = r[k]
        base["static_" + name] = dict(off=r["off"], spatial=r["spatial"])
    print("baselines:", json.dumps(base))
    print("%-26s %9s %9s %9s %9s %9s %9s" % ("point", "rest st", "rest or", "box st", "box or", "static or", "static st"))
    for k, v in rows.items():
        print("%-26s %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f" % (k, v["rest_still"], v["rest_orbit"], v["box_follow_still"], v["box_follow_orbit"], v["static_orbit"], v["static_still"]))
    ok = [k for k, v in rows.items() if v["static_orbit"] < base["static_orbit"]["spatial"]]
    best = min(ok, key=lambda k: rows[k]["rest_still"] + rows[k]["rest_orbit"])
    print("choice:", best, json.dumps(rows[best]))
    if "--json" in sys.argv:
        json.dump(dict(baselines=base, grid=rows, choice=best, offsets=offsets), open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
