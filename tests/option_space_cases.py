"""The ReSTIR option sets past the reference's defaults, one table for the CPU test (tests/test_option_space_cpu.py: the oracle alone,
what keeps the cases from being trivial) and the GPU tests (tests/test_gpu_option_space.py: the device against the oracle).

Every case is `name -> (group, W, H, optkw, branch)`: the option set goes on top of `bench_options()` (temporal + spatial reuse on, 32
candidates, 5 neighbours, radius 30, 3 passes), the scene is `scenes.make_quad_room()` seen from EYE towards LOOKAT, 3 frames.
`branch` says which host- or device-side branch of the library the case is there for (csrc/restir_rt.hip, csrc/frame_kernels.h,
csrc/frame_roles.h).
"""
EYE, LOOKAT = (0.5, 2.5, 6.0), (0.0, 1.5, -1.0)
FRAMES = (1, 2, 3)

S = dict(use_shadowed_target_function=1)

CASES = {
    # ---- spatial passes: pass index 3 and above (frame_roles.h roles_pass ping-pong, rt_ray_count's per-pass replay)
    "passes4": ("passes", 80, 45, dict(spatial_resampling_passes=4),
                "roles_pass index 3 (even pass count: the frame ends in RT_RES_0), unshadowed cooperative gather"),
    "passes5": ("passes", 80, 45, dict(spatial_resampling_passes=5),
                "roles_pass indices 3 and 4 (odd count: the frame ends in RT_RES_1)"),
    "passes8_n2": ("passes", 80, 45, dict(spatial_resampling_passes=8, spatial_resampling_sample_count=2),
                   "roles_pass indices 3..7: the pass count rt_mg's arenas are sized for"),
    "passes4_shadowed": ("passes", 80, 45, dict(S, spatial_resampling_passes=4),
                         "pass index 3 of the shadowed target's batched (<= 5 neighbours) form, its rays in rt_ray_count"),
    "passes5_shadowed_n6_r45": ("passes", 80, 45, dict(S, spatial_resampling_passes=5, spatial_resampling_sample_count=6, spatial_resampling_radius=45.0),
                                "pass indices 3, 4 of the shadowed target's one-ray form (> 5 neighbours) at a reach of 130 px"),
    "passes25_ris1_n1": ("passes", 80, 45, dict(spatial_resampling_passes=25, ris_sample_count=1, spatial_resampling_sample_count=1),
                         "the largest pass count rt_options_set accepts (its bound on M, 21 * 2^25, is below 2^30): pass indices 3..24"),
    # ---- radius: halo_rows_needed and everything keyed on SPL_HALO = 87
    "radius0": ("radius", 80, 45, dict(spatial_resampling_radius=0.0),
                "scale 0: every neighbour is the pixel itself and is skipped"),
    "radius0_5": ("radius", 80, 45, dict(spatial_resampling_radius=0.5),
                  "a reach below one pixel: only the truncation of a negative offset leaves the pixel"),
    "radius31": ("radius", 80, 45, dict(spatial_resampling_radius=31.0),
                 "halo_rows_needed = 90 > SPL_HALO: the first radius past the windowed forms"),
    "radius45": ("radius", 80, 45, dict(spatial_resampling_radius=45.0),
                 "halo_rows_needed = 130: most neighbours of a 45-row image fall outside it"),
    "radius200": ("radius", 80, 45, dict(spatial_resampling_radius=200.0),
                  "halo_rows_needed = 577: nearly every draw is off the image"),
    "radius90_tall": ("radius_tall", 64, 540, dict(spatial_resampling_radius=90.0),
                      "halo_rows_needed = 260 on an image tall enough for the neighbours to land on it"),
    # ---- neighbours per pass: the batched forms (<= 5), the one-ray forms, the mark's quick reject (1..8)
    "neighbours0": ("neighbours", 80, 45, dict(spatial_resampling_sample_count=0),
                    "no neighbour loop at all: halo_rows_needed = 0, the pass hands its input on"),
    "neighbours6": ("neighbours", 80, 45, dict(spatial_resampling_sample_count=6),
                    "the first count past the five-neighbour batched gather (frame_kernels.h spatial forms)"),
    "neighbours8": ("neighbours", 80, 45, dict(spatial_resampling_sample_count=8),
                    "the last count for which the mark's quick reject applies"),
    "neighbours9": ("neighbours", 80, 45, dict(spatial_resampling_sample_count=9),
                    "nine neighbours: past the quick reject; rt_ray_count / rt_spatial_bytes replay 9 draws per pass"),
    "neighbours16_p1": ("neighbours", 80, 45, dict(spatial_resampling_sample_count=16, spatial_resampling_passes=1),
                        "sixteen neighbours in one pass"),
    "neighbours6_shadowed": ("neighbours", 80, 45, dict(S, spatial_resampling_sample_count=6),
                             "shadowed target, the one-ray form right past the batched one (k_spatial<true, false>)"),
    "neighbours9_shadowed": ("neighbours", 80, 45, dict(S, spatial_resampling_sample_count=9),
                             "shadowed target, nine neighbours: 10 shadow rays per pixel and pass in rt_ray_count"),
    # ---- candidates per pixel
    "ris0": ("candidates", 80, 45, dict(ris_sample_count=0),
             "no candidate: every reservoir stays empty (M = 0) through temporal and spatial reuse"),
    "ris1": ("candidates", 80, 45, dict(ris_sample_count=1), "one candidate: the candidate loop runs once, the temporal cap is 20"),
    "ris31": ("candidates", 80, 45, dict(ris_sample_count=31), "31 candidates: an odd count just below the default, three full batches of 8 and a partial one where batched"),
    "ris33": ("candidates", 80, 45, dict(ris_sample_count=33), "33 candidates: one past four full batches of 8; temporal cap 660"),
    "ris64": ("candidates", 80, 45, dict(ris_sample_count=64), "64 candidates, twice the default: temporal cap 1280"),
    "ris100": ("candidates", 80, 45, dict(ris_sample_count=100), "100 candidates, no multiple of 8: temporal cap 2000"),
    "ris33_shadowed": ("candidates", 80, 45, dict(S, ris_sample_count=33),
                       "shadowed target: 33 candidate shadow rays per pixel in generate_candidate and in rt_ray_count"),
}

NO_MERGE = ("radius0", "neighbours0")  # the spatial passes leave M as temporal reuse left it
# A draw lands on the 80x45 image with probability below W * H / (2 pi (200 / 1.96)^2) = 0.055 (the Gaussian's peak density times the
# image's area), so with 15 draws per frame fewer than 1 - 0.945^15 = 57 % of the pixels merge at the image centre and fewer towards
# its edges: the MEDIAN pixel need not merge. Some pixels must: the expected number of landing draws is in the hundreds per frame.
SPARSE_MERGE = ("radius200",)
KERNEL_SEQUENCE_GROUPS = ("passes", "neighbours", "candidates")


def names(groups=None):
    return [n for n, c in CASES.items() if groups is None or c[0] in groups]
