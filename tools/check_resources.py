#!/usr/bin/env python3
"""Register / spill / occupancy check of the frame kernels (RT_RESOLVE_WAVES 8 and RT_SHSPATIAL_WAVES 7 fit without
spilling only because of -fno-slp-vectorize; another hipcc or EXTRA flag could spill again — correct results, large slow-down).

csrc/Makefile compiles restir_rt.hip with -Rpass-analysis=kernel-resource-usage (remarks only: the code is the same) and keeps
the remarks in build/resource_usage.log; this script turns them into a table (stdout, `--table FILE`) and FAILS (exit 1) when a
kernel named in BUDGET spills more vector registers or holds fewer wavefronts per SIMD than recorded here.

  python tools/check_resources.py cedec_2024_rt_amd/csrc/build/resource_usage.log [--table profiles/r05_kernel_resources.txt]
"""
import re
import subprocess
import sys

from kernel_forms import ANY, generate_candidate as gc, temporal as kt

# kernel (demangled name up to the argument list, regex) -> (max spilled VGPRs, min wavefronts per SIMD)
# numbers = the build of round 5 (hipcc of ROCm 7.2.0, csrc/Makefile flags); the shadowed pass is the one kernel that is
# ALLOWED to spill (72 VGPRs + spills at 7 wavefronts per SIMD beat 112 VGPRs at 4: docs/MEASUREMENT_LOG_r04.md section 9)
BUDGET = [
    (r"^k_raycast<false>", 0, 8),
    (r"^k_raycast<true>", 0, 7),                                              # strips: work-sharing closest-hit walk
    ("^" + gc(fuse=1, ws=1, raycast=1, power=ANY, grid=ANY), 0, 6),                          # the whole frame's stage 0: primary ray + candidates + temporal
    ("^" + gc(fuse=1, ws=1, power=ANY, grid=ANY), 0, 6),                                     # candidates + temporal (strips, rt_timing)
    ("^" + gc(fuse=1, power=ANY, grid=ANY), 0, 5),                                           # ... without the work-sharing walk (rt_tuning 13 = 0)
    ("^" + gc(power=ANY, grid=ANY), 0, 6),                                                   # rt_generate_candidate
    # r23 rt_temporal_reprojection: the fused forms with the history gathered by reprojection (last argument), uniform and power lights
    ("^" + gc(fuse=1, ws=1, raycast=1, power=ANY, reproject=1, grid=ANY), 0, 6),             # one-launch stage 0: 79 VGPRs as the default form
    ("^" + gc(fuse=1, ws=1, power=ANY, reproject=1, grid=ANY), 0, 6),                        # candidates + temporal: 79
    ("^" + gc(fuse=1, power=ANY, reproject=1, grid=ANY), 0, 5),                              # without the work-sharing walk: 82
    ("^" + gc(fuse=1, shadowed=1, power=ANY, reproject=1, grid=ANY), 0, 4),                  # shadowed target function: 109
    ("^" + kt(reproject=1), 0, 7),                                                           # rt_temporal_resampling: 66
    ("^" + kt(shadowed=1, reproject=1), 0, 4),                                               # ... shadowed: 113
    # r24 rt_temporal_motion: the same forms with the history that follows moved triangles (last argument), uniform and power lights
    ("^" + gc(fuse=1, ws=1, raycast=1, power=ANY, reproject=1, motion=1, grid=ANY), 0, 6),   # one-launch stage 0
    ("^" + gc(fuse=1, ws=1, power=ANY, reproject=1, motion=1, grid=ANY), 0, 6),              # candidates + temporal
    ("^" + gc(fuse=1, power=ANY, reproject=1, motion=1, grid=ANY), 0, 5),                    # without the work-sharing walk
    ("^" + gc(fuse=1, shadowed=1, power=ANY, reproject=1, motion=1, grid=ANY), 0, 4),        # shadowed target function
    ("^" + kt(reproject=1, motion=1), 0, 7),                                                 # rt_temporal_resampling
    ("^" + kt(shadowed=1, reproject=1, motion=1), 0, 4),                                     # ... shadowed
    (r"^k_temporal_unbiased", 0, 4),     # r31 rt_temporal_unbiased: 101 VGPRs without a budget, no spill (budget 5: 95, no spill; 6: 80 and 15 spilled)
    # r33 rt_light_grid: the last argument of every k_generate_candidate entry above; the grid forms hold their neighbours' budgets, and
    # the shadowed form without reprojection, in both
    ("^" + gc(fuse=1, shadowed=1, grid=ANY), 0, 4),
    ("^" + gc(shadowed=1, grid=ANY), 0, 4),
    (r"^k_spatial_coop<6, false, 256>", 0, 6),                                # the roofline kernel
    (r"^k_spatial_coop<6, true, 256>", 0, 5),                                 # strips: halo lists read / written in the pass
    (r"^k_resolve<", 0, 8),
    (r"^k_spatial<true, true>", 80, 7),
    (r"^k_spatial_unbiased", 0, 4),      # r15 rt_spatial_unbiased: 124 VGPRs, no spill at 4 wavefronts per SIMD (5 / 6 / 7: 93 / 171 / 164 spilled)
    (r"^k_tone_mapping", 0, 8),
    (r"^k_halo_mark<", 0, 8),
    (r"^k_ao<0>", 0, 7),   # r07 ambient occlusion, pixel-major (default): 8 wavefronts per SIMD (RT_AO_WAVES=8) measured no faster
    (r"^k_ao<1>", 0, 6),   # ray-major (rt_tuning 27 = 1)
    (r"^k_denoise_guide<false>", 0, 8),  # r09 rt_denoise: primary rays of the guide (k_raycast's walk)
    (r"^k_denoise_guide<true>", 0, 6),
    (r"^k_denoise_demod", 0, 8),
    (r"^k_denoise_var", 0, 8),
    (r"^k_denoise_iter<", 0, 8),         # a-trous level, per-lane gathers (rt_tuning 28 = 0)
    (r"^k_denoise_iter_lds<", 0, 8),     # residue lattice in LDS (rt_tuning 28 = 1), 19 200 B per workgroup
    (r"^k_denoise_output", 0, 8),
    (r"^k_denoise_temporal", 0, 8),      # r10 rt_denoise_temporal: reprojection + integration
    (r"^k_denoise_var_hist", 0, 8),      # variance with history
    # r30 rt_denoise_temporal_antilag: dn_temporal_pixel up to the blend (41 VGPRs as its siblings), and the window kernel, 12 800 B of LDS
    (r"^k_denoise_antilag_gather<", 0, 8),
    (r"^k_denoise_antilag$", 0, 8),
    (r"^k_denoise_temporal_motion", 0, 8),  # r25 rt_denoise_temporal_motion: the followed call's form, 41 VGPRs / 46 SGPRs (its sibling: 41 / 44)
    # r32 rt_temporal_light_motion: the re-basing pass of rt_scene_update
    (r"^k_light_follow<true>", 0, 8),    # loop over the span's lights: 49 VGPRs
    # r36 rt_indirect: 08_nee's depth loop from the G-buffer, at 08_nee's budget (k_path_trace<8>: 80 VGPRs, 15 spilled)
    (r"^k_indirect$", 14, 6),            # one launch: 80 VGPRs, 14 spilled (budget 5: 96, none; 7: 72, 23; 8: 64, 36)
    (r"^k_light_follow<false>", 0, 7),   # point query on the old tree: 66 VGPRs, 14 336 B of LDS (the stack), 208 B of scratch (its overflow, as trace_wide)
]


def parse(path):
    txt = open(path, errors="replace").read()
    rows = []
    names = []
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        names.append(b.split()[0])
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for b, d in zip(re.split(r"remark: Function Name: ", txt)[1:], dem):
        g = lambda k: int(re.search(k + r": (\d+)", b).group(1))  # noqa: E731
        # strip the argument list, keep the template arguments
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        name = d[:cut].replace("void ", "").replace("rt::", "")
        rows.append(dict(name=name, vgpr=g("VGPRs"), agpr=g("AGPRs"), sgpr=g("TotalSGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                         occ=g(r"Occupancy \[waves/SIMD\]"), spill=g("VGPRs Spill"), sspill=g("SGPRs Spill"), lds=g(r"LDS Size \[bytes/block\]")))
    return rows


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    rows = parse(sys.argv[1])
    if not rows:
        raise SystemExit("no kernel-resource-usage remarks in " + sys.argv[1])
    lines = ["%-86s VGPR AGPR SGPR scratch occ spillV spillS   LDS" % "kernel"]
    seen = {}
    for r in rows:
        if r["name"] in seen or "rocprim" in r["name"]:  # the library's sort / scan kernels (BVH build) are not ours to budget
            continue
        seen[r["name"]] = r
        lines.append("%-86s %4d %4d %4d %7d %3d %6d %6d %5d" % (r["name"][:86], r["vgpr"], r["agpr"], r["sgpr"], r["scratch"], r["occ"], r["spill"], r["sspill"], r["lds"]))
    bad = []
    for pat, max_spill, min_occ in BUDGET:
        hit = [r for r in seen.values() if re.search(pat, r["name"])]
        if not hit:
            bad.append("no kernel matches %r (renamed? update tools/check_resources.py)" % pat)
        for r in hit:
            if r["spill"] > max_spill or r["occ"] < min_occ:
                bad.append("%s: %d spilled VGPRs (budget %d), %d wavefronts per SIMD (budget >= %d)" % (r["name"], r["spill"], max_spill, r["occ"], min_occ))
    table = "\n".join(lines) + "\n"
    if "--table" in sys.argv:
        open(sys.argv[sys.argv.index("--table") + 1], "w").write(table)
    elif "--quiet" not in sys.argv:
        sys.stdout.write(table)
    if bad:
        sys.stderr.write("kernel resource budget exceeded (tools/check_resources.py):\n  " + "\n  ".join(bad) + "\n")
        raise SystemExit(1)


if __name__ == "__main__":
    main()
