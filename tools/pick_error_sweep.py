"""GPU. Where the bound E of csrc/neighbour_pick.h comes from: the fast functions of the neighbour pick against the exact ones over
EVERY input. Both draws of a pick are k * 2^-23, k = 0 .. 2^23 - 1 (PCG::uniformf), so there are 2^23 arguments each:

  rv0:  radius' = sqrt(log2(rv0) * (-2 ln 2)) on the hardware's v_log_f32 / v_sqrt_f32   against   sqrt_guarded(fmax(-2 pm_logf(rv0), 0))
  rv1:  v_sin_f32 / v_cos_f32 of rv1 (revolutions)                                       against   pm_sincosf(2 pi rv1)

through rt_math_eval functions 39 .. 44 (k_math_eval, frame_kernels.h). Prints one JSON line: the maximum absolute differences Er, Es,
Ec (and where), the largest finite radius Rmax, how many arguments gave a non-finite fast value (rv0 = 0 only), the constants the header
holds, and whether they are at least twice the measured maxima. docs/MEASUREMENT_LOG_r22.md section 2 records a run.

  python tools/pick_error_sweep.py [--chunk 2097152]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def header_constants():
    src = open(os.path.join(ROOT, "cedec_2024_rt_amd", "csrc", "neighbour_pick.h")).read()
    er = float(re.search(r"kPickEr = 2\.0f \* ([0-9.e+-]+)f;", src).group(1))
    em = float(re.search(r"kPickEm = 2\.0f \* ([0-9.e+-]+)f;", src).group(1))
    rmax = float(re.search(r"kPickRmax = ([0-9.e+-]+)f;", src).group(1))
    return dict(kPickEr=2 * er, kPickEm=2 * em, kPickRmax=rmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=1 << 21)
    args = ap.parse_args()
    from cedec_2024_rt_amd import api

    r = api.Renderer(64, 48)
    N = 1 << 23
    worst = dict(Er=(0.0, 0), Es=(0.0, 0), Ec=(0.0, 0))
    rmax, nonfinite_r, nonfinite_sc = 0.0, 0, 0
    for k0 in range(0, N, args.chunk):
        k = np.arange(k0, min(k0 + args.chunk, N), dtype=np.uint32)
        rv = (k.astype(np.float64) * 2.0 ** -23).astype(np.float32)  # exact: k < 2^24
        fast_r, exact_r = r.math_eval(39, rv).astype(np.float64), r.math_eval(40, rv).astype(np.float64)
        fin = np.isfinite(exact_r) & np.isfinite(fast_r)
        nonfinite_r += int((~fin).sum())
        # wherever the exact radius is finite the fast one must be too (else the guard sends the lane to the exact path: harmless, but it must be rv0 = 0 only)
        assert not (np.isfinite(exact_r) & ~np.isfinite(fast_r) & (k > 0)).any(), "a non-finite fast radius for rv0 > 0"
        d = np.where(fin, np.abs(fast_r - exact_r), 0.0)
        i = int(d.argmax())
        if d[i] > worst["Er"][0]:
            worst["Er"] = (float(d[i]), int(k[i]))
        rmax = max(rmax, float(exact_r[fin].max()))
        for name, ff, fe in (("Es", 41, 43), ("Ec", 42, 44)):
            a, b = r.math_eval(ff, rv).astype(np.float64), r.math_eval(fe, rv).astype(np.float64)
            nonfinite_sc += int((~np.isfinite(a)).sum() + (~np.isfinite(b)).sum())
            d = np.abs(a - b)
            i = int(d.argmax())
            if d[i] > worst[name][0]:
                worst[name] = (float(d[i]), int(k[i]))
    r.close()
    hc = header_constants()
    out = dict(arguments=N, Er=worst["Er"][0], Er_at_k=worst["Er"][1], Es=worst["Es"][0], Es_at_k=worst["Es"][1], Ec=worst["Ec"][0], Ec_at_k=worst["Ec"][1],
               Rmax=rmax, nonfinite_radius_arguments=nonfinite_r, nonfinite_sincos=nonfinite_sc, header=hc,
               header_is_twice_the_maxima=bool(hc["kPickEr"] >= 2 * worst["Er"][0] and hc["kPickEm"] >= 2 * max(worst["Es"][0], worst["Ec"][0]) and hc["kPickRmax"] >= rmax))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
