/*
 * restir_rt.hip — the C-ABI of include/restir_rt.h: context, scene/BVH set-up, camera, options,
 * one launch wrapper per reference kernel, the staged frame, host<->device conversion, halo calls
 * and measurement. The only translation unit of librestir_rt.so; it includes
 *   frame_kernels.h    every device kernel (32x8-pixel tiles, XCD-banded workgroup order)
 *   bvh.h              device LBVH build kernels + both traversals
 *   bvh_build_host.h   reference pre-split, SAH builder, wide-BVH collapse
 *   rt_device.h        vector math, PCG, the reference's pure functions, HBM record layouts
 * Compile with -ffp-contract=off (parity contract, rt_device.h).
 */
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/restir_rt_internal.h"
#include "bvh.h"
#include "frame_roles.h"
#include "history_provenance.h"
#include "stage0_forms.h"
#include "rt_device.h"

using namespace rt;

static_assert(sizeof(rt_triangle) == 60, "Triangle layout (common/core.hpp:38-43)");
static_assert(sizeof(rt_visibility) == 16, "Visibility layout (common/core.hpp:167-172)");
static_assert(sizeof(rt_reservoir) == 76, "Reservoir layout (common/reservoir.hpp:5-38)");
static_assert(sizeof(rt_options) == 48, "Options layout (common/options.hpp:4-22)");
static_assert(offsetof(rt_options, use_shadowed_target_function) == 44, "Options layout");
static_assert(sizeof(rt_raygen) == 36, "RayGenerator layout (common/camera.hpp:5-9)");
static_assert(sizeof(BvhNode) == 64, "BVH node");
static_assert(ROLE_RES_0 == RT_RES_0 && ROLE_RES_1 == RT_RES_1 && ROLE_RES_TEMPORAL == RT_RES_TEMPORAL, "frame_roles.h names the reservoir buffers as restir_rt.h does");

#include "neighbour_pick.h"
#include "frame_kernels.h"
#include "host_path.h"
#include "bvh_build_host.h"
#include "bvh_build_device.h"
#include "bvh_refit.h"
#include "denoise_kernels.h"
#include "light_follow_kernels.h"

/* ======================================================================= host */

struct rt_ctx
{
    int device = 0, W = 0, H = 0, row_begin = 0, row_end = 0, halo = 0;
    int lrow0 = 0, lrows = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    /* second lane of a frame stage (rt_frame_stage_run_async): interior rows run beside the boundary rows */
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_stage = nullptr, ev_aux = nullptr;
    bool aux_used = false;
    /* The raycast of frame f+1 does not depend on frame f (it needs the camera only), so rt_frame_stage launches it on a
     * stream of its own behind stage 0 of frame f, into the second G-buffer set: it runs beside the spatial passes
     * (HBM-bound) and the halo exchanges of frame f and frame f+1 starts at generate_candidate. The result is used only
     * if nothing it depends on changed meanwhile (epoch: camera, scene, options); otherwise frame f+1 traces its
     * primary rays as usual. rt_tuning key 14. */
    struct
    {
        hipStream_t stream = nullptr;
        hipEvent_t ev_go = nullptr, ev_done = nullptr, ev_t[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
        int timed_set = -1;
        bool valid = false, timed[3] = {false, false, false};
        bool outstanding = false; /* work recorded by ev_done that the main stream has not waited for yet */
        bool reuse = false;       /* it read the current G-buffer set (gbuffer_reusable): candidates only, no primary rays */
        /* its candidates (pipelined stage 0, further down): for which frame, from which history buffer, under which tag (below) */
        bool gen_valid = false;
        int gen_frame = 0, gen_hist = -1;
        uint32_t gen_tag = 0;
        uint64_t epoch = 0, res_epoch = 0; /* `epoch` / `res_epoch` of the context when it was launched */
    } ahead;
    /* r05: THREE G-buffer sets (frame f reads set f mod 3): the pipelined stage 0 of frame f+1 overwrites the set of frame f-2,
     * whose last reader — resolve(f-2) — is two tails back, not the set resolve(f-1) may still be reading (with two sets every
     * look-ahead raycast waited for the previous frame's resolve: the one edge that made a strip's frame a dependency chain
     * instead of three streams of independent work, profiles/r05_strip_timelines.txt) */
    static constexpr int NGSET = 3;
    struct
    {
        float4* set[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}; /* [set]{vis, g0, g1}; vis/g0/g1 = set cur */
        int cur = 0;
        float4 *vis = nullptr, *g0 = nullptr, *g1 = nullptr;
        bool valid = false, shaded_bits_stale = true; /* a G-buffer has been traced or uploaded / d_shaded_bits predates it */
        /* which G-buffer a reservoir buffer's shaded bits belong to (k_refresh_shaded, HistoryTag::gserial): serial counts G-buffer writes; epoch: the one the current G-buffer was traced under */
        uint64_t serial = 0, epoch = 0;
        /* r13, rt_gbuffer_reuse: the primary ray of a pixel has no jitter and no frame number in it (frame_kernels.h, shoot(xi / W, yi / H)),
         * so Visibility / g0 / g1 are a function of camera, scene and image size: of `epoch`. A staged frame of a whole-frame context whose
         * current set was traced over all owned rows under the current epoch launches its candidates on that set and no primary rays
         * (gbuffer_reusable). traced_epoch: the epoch under which ALL owned rows of set cur were traced by a raycast launch or the
         * one-launch stage 0 (0 = never; an upload bumps `epoch` and does not set it: k_gbuffer_from_vis is not a trace).
         * ahead_ordered: ahead.stream is known to be behind the launch that wrote the set (the look-ahead candidates read it there). */
        bool reuse = true, ahead_ordered = false;
        uint64_t traced_epoch = 0, primary_launches = 0;
    } gbuf;
    /* tags of the own-visibility flags (rt_device.h): one number per staged frame and per pipelined stage 0; the launches of
     * a staged frame carry frame.tag (Launch::tag), the per-kernel entry points carry 0 */
    uint32_t ownv_serial = 0;
    /* history_provenance.h. res_tag: what each physical reservoir buffer was last written under, kept whether a mode is on or not
     * (r23, rt_temporal_reprojection, DESIGN.md section 13: a temporal merge whose history buffer carries another camera than the
     * current one launches the REPROJECT kernels while the mode is on, history_camera), and the G-buffer its shaded bits belong to.
     * moved: the geometry generation, both motion toggles and the moved range (r24, rt_temporal_motion, section 14; r25,
     * rt_denoise_temporal_motion, section 15); d_tv_prev (layout of d_tv) holds the kept vertices while moved.kept. */
    HistoryTag res_tag[5];
    bool reproject = false;
    bool temporal_unbiased = false; /* rt_temporal_unbiased (r31, section 20): a reprojecting merge normalises by 1/Z (k_temporal_unbiased) */
    MovedGeometry moved;
    float4* d_tv_prev = nullptr;
    /* rt_temporal_light_motion (r32, light_follow.h): the toggle; spans of at most lf_direct_max old lights take
     * the direct loop, larger ones the point query on the old tree; d_lf_words: the device counters (LF_COUNTER_WORDS of 64 bit), then the six
     * words of the early-out box; d_lf_stage: the span's new triangles and old light ids during an update; lf_stats[0]: buffers
     * re-based since the toggle went on (the other four are the device counters); lf_last: buffers the last update re-based */
    bool light_follow = false;
    int lf_direct_max = LF_DIRECT_MAX_DEFAULT;
    int lf_last = 0;
    uint64_t lf_stats0 = 0;
    unsigned long long* d_lf_words = nullptr;
    void* d_lf_stage = nullptr;
    size_t lf_stage_bytes = 0;
    hipEvent_t lf_ev[2] = {nullptr, nullptr};
    bool lf_timed = false, lf_launched = false;
    unsigned long long* d_walk = nullptr; /* rt_walk_stats: 4 kernel slots x 4 counters, then the slot of rt_occluder_hint_stats (WALK_SLOTS) */
    bool walk_on = false;
    /* r19, rt_occluder_hints: OCCLUDER_HINTS triangle indices per pixel of the local rows (occluder_hint.h), the triangles that occluded
     * the pixel's earlier candidate rays. Made at the first staged frame, all -1 then and after every rt_scene_set (the triangle count
     * can shrink); rt_scene_update leaves it (an index stays an index of the scene). Read and written by the staged frame's candidates
     * only: the per-kernel entry point passes none. */
    int* d_hints = nullptr;
    bool hints_on = true;
    int tune_ws_primary = -1; /* rt_tuning key 16: primary rays with the work-sharing closest-hit walk: -1 auto (r04) = launches of at
                                 most about one generation of wavefronts (a 135-row strip: -1.5 % of its frame; whole frames +2 %), 0 never, 1 always */
    int tune_stream = 0; /* rt_tuning key 15: resolve as a stream of pixels through persistent wavefronts (A/B: slower) */
    int n_cus = 256;
    int tune_spec = -1; /* rt_tuning key 14: -1 auto = strip contexts: primary rays AND candidates of the next frame, 0 never,
                           1 = the next frame's primary rays only, 2 = primary rays and candidates */
    bool lane_saved = false, lane_timing = false; /* rt_lane */
    hipStream_t lane_main = nullptr;
    std::string err;

    int n_tris = 0, n_lights = 0, bvh_height = 0, n_refs = 0;
    /* rt_tuning: tile order per kernel {raycast, generate, spatial, resolve, other} and the spatial
     * pass's occupancy limiter (extra dynamic LDS). Defaults from the sweep in DESIGN.md §5. */
    int tune_tile_mode[5] = {-1, -1, -1, -1, 0}; /* -1 = auto (make_params): r05 — the tracing kernels take their tiles INTERLEAVED over
                                                    the XCDs (whole frames: tile rows k, k + 8, ...; strips: tile b on XCD b % 8), the
                                                    spatial pass keeps an XCD's band of tile rows, column by column (its +-87-px
                                                    neighbour window must stay in that XCD's L2); profiles/r05_tile_interleave_ab.txt */
    int tune_spatial_lds = 0;     /* rt_tuning key 4: extra dynamic LDS per unshadowed spatial workgroup (A/B of the old throttle) */
    int pick_mode = PICK_FAST; /* rt_neighbour_pick (r22): k_spatial_coop's neighbour pick, neighbour_pick.h; the same integers in every mode */
    int tune_spatial_variant = 2; /* rt_tuning key 8: 2 = k_spatial_coop (default: four lanes per record, LDS-DMA gathers, transposed
                                     stores), 0 = k_spatial_gather (one per-lane gather per neighbour), 1 = k_spatial_lds (staged
                                     shaded-bit window; falls back to 0 where it does not apply) */
    int tune_spatial_waves = -1;  /* rt_tuning key 9: register budget of the unshadowed spatial pass in wavefronts per SIMD: 4, 5, 6, 0 = what the
                                     kernel needs (7), -1 = auto: 4 for the gather kernel (its neighbour window must stay in L2: 0.184 vs 0.202 ms
                                     per pass), none for the LDS-staged kernel (0.181 ms unbounded, 0.188 at 4) — profiles/r02_spatial_variants.json */
    uint32_t* d_shaded_bits = nullptr;
    uint32_t* d_mark_bits = nullptr; /* rt_halo_mark (key 19): shaded bits of all local rows, rebuilt per mark */
    /* deferred visibility-reuse rays of the fused candidate kernel (frame_kernels.h, DEFER): one queue per lane
     * (main / second stream), its counter, and the last count that reached the host (sizes the next launch) */
    int tune_defer_vis = 0; /* rt_tuning key 11 */
    int tune_ris_pipe = 0;  /* rt_tuning key 12: software-pipelined RIS loop in the fused unshadowed candidate kernel */
    int tune_ws = 1;        /* rt_tuning key 13: work-sharing shadow-ray walk in generate / resolve: -1 auto (launches of
                               at most RT_WS_AUTO_WAVES wavefronts), 0 never, 1 always */
    uint32_t* d_visq[2] = {nullptr, nullptr};
    unsigned int* d_visq_count = nullptr; /* [2] */
    unsigned int* h_visq_count = nullptr; /* pinned [2]; 0xffffffff = unknown */
    uint64_t visq_epoch = 0;
    float last_trace_ms = 0.0f;
    int last_frame = 0; /* frame number of the last rt_frame_stage / rt_spatial_resampling (ray counting) */
    int trace_mode = 0; /* rt_trace_closest / rt_trace_stats: 0 = wide (what the frame kernels use), 1 = binary stackless */
    float bvh_split_factor = 10.0f; /* fragment length in median triangle extents; 0 = no pre-split */
    int bvh_bfs_records = 2048; /* rt_tuning key 7: records emitted breadth-first (top of the tree contiguous) */
    int bvh_builder = 3; /* 0 = device LBVH (Morton/Karras, host pre-split + collapse), 1 = host binned SAH (high quality), 2 = device: pre-split, PLOC,
                            host SAH sweep over the top, wide collapse, 3 (default, r03) = device: pre-split, top-down binned SAH (the host builder's
                            algorithm and tree), wide collapse */
    float build_ms = 0.0f; /* wall time of the last rt_scene_set */
    int ploc_radius = RT_PLOC_RADIUS; /* rt_tuning key 10 */
    float* d_tris = nullptr;
    float4* d_tv = nullptr;
    BvhNode* d_nodes = nullptr;
    float4* d_wide = nullptr;
    int n_wide = 0, wide_height = 0;
    float4* d_trimat = nullptr;
    float4* d_lights = nullptr;
    float4* d_light_ke = nullptr;
    /* rt_scene_update: the light list in index order (host), its device copy, the refit's level lists (built at the first
     * update of a scene: refit_off[l] .. refit_off[l + 1] = inner records of level l), its box scratch and the scene bounds */
    std::vector<uint32_t> h_lights;
    /* rt_light_sampling (light_alias.h): the mode, per-light host weights (so that rt_scene_update needs only its
     * span), the alias table with its realised counts, and on the device the table and a second light table whose pdf is the realised one */
    int light_mode = RT_LIGHTS_UNIFORM;
    std::vector<float> h_light_w;
    std::vector<AliasSlot> h_alias;
    std::vector<uint64_t> h_alias_K;
    bool alias_ok = false; /* some light has q > 0 */
    float4* d_lights_power = nullptr;
    AliasSlot* d_alias = nullptr;
    /* rt_light_grid (light_grid.h): the request (0 cells = off), and only while it is on: a host copy of the
     * scene's triangles (the bounds need every vertex, the runs the lights' vertices; rt_scene_update passes its span only), the
     * tables as the host built them and their device copies with a light table and a Ke table in the runs' position order */
    int grid_cells = 0, grid_clusters = 0;
    std::vector<float> h_grid_tris; /* 15 floats per triangle */
    LightGrid h_grid;
    bool grid_built = false;
    AliasSlot* d_grid_cells = nullptr;
    float* d_grid_cell_prob = nullptr;
    GridRun* d_grid_runs = nullptr;
    AliasSlot* d_grid_run_slots = nullptr;
    uint32_t* d_grid_cluster_of = nullptr;
    float4* d_lights_grid = nullptr;
    float4* d_light_ke_grid = nullptr;
    float grid_build_ms = 0.0f; /* the last build, host tables and upload */
    uint32_t* d_light_ids = nullptr;
    uint32_t* d_refit_list = nullptr;
    float* d_refit_box = nullptr;
    unsigned int* d_refit_bounds = nullptr;
    std::vector<uint32_t> refit_off;
    /* fragments of pre-split triangles (bvh_refit.h): frag_pending = the device build left fragment numbers in the leaves and
     * the table is still to be made (at the first update, from the build's triangles, fragment length and pad); then the
     * vertex-major (u, v) table and the vertex counts of n_frags fragments. cost_at_build: rt_bvh_cost of the tree before
     * its first refit (< 0: not taken yet) */
    bool frag_pending = false;
    float frag_L = 0.0f, frag_pad = 0.0f;
    float* d_frag_uv = nullptr;
    uint8_t* d_frag_n = nullptr;
    uint32_t n_frags = 0;
    double cost_at_build = -1.0;
    bool bin_stale = false; /* the binary tree (d_nodes, trace mode 1 of the experiments library) predates an update */

    float4* d_accum = nullptr;
    uint32_t* d_pixels = nullptr;
    float4* d_rec[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; /* the five reservoir buffers; their roles: frame (frame_roles.h) */
    float4* d_rad[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    /* Pipelined stage 0 (rt_tuning key 14 = 2, r03): frame f+1's generate_candidate(+temporal_resampling) depends on frame
     * f only through the temporal history, and the reference saves that history right after temporal_resampling, BEFORE
     * the spatial passes (10_restir_di.cpp:314-321) — so stage 0 of frame f+1 (primary rays, candidates, temporal merge)
     * can run beside the spatial passes, halo exchanges and resolve of frame f. It is launched on ahead.stream behind
     * stage 0 of frame f, reads the history frame f just wrote, writes the spare buffer, and frame f+1 takes it if it
     * is frame f+1 indeed and nothing it read has changed meanwhile (epoch: camera / scene / options / uploads;
     * res_epoch: any call that writes a reservoir buffer outside the staged frame). Same launches, same results. */
    /* Tail stream (rt_tuning key 17, r03): resolve + tone_mapping of frame f read only frame f's final reservoirs and
     * G-buffer, so a strip's main stream does not wait for them — it goes on with frame f+1's first halo exchange while
     * they run on a stream of their own. Whatever could overwrite what they read waits for tail.ev first: the next frame's
     * first spatial pass (its output buffer can be this frame's final one), the next-but-one frame's pipelined stage 0 (same
     * G-buffer set, spare reservoir buffer), and every call outside the staged frame (join_tail). */
    struct
    {
        hipStream_t stream = nullptr;
        hipEvent_t ev_go = nullptr, ev = nullptr;
        /* ev_resolved[0] = behind the latest staged frame's resolve (+ tone mapping) on whatever stream it ran, [1] = the one before:
         * what the pipelined stage 0 waits for before it overwrites the G-buffer set and the reservoir buffer of two frames ago */
        hipEvent_t ev_resolved[2] = {nullptr, nullptr};
        int n_resolved = 0;
        bool resolve_on = false; /* the running frame's resolve went to the tail stream */
        bool pending_main = false;
        int phys = -1; /* reservoir buffer the tail in flight reads (the frame's final one) */
    } tail;
    int tune_tail = -1; /* -1 auto = on, 0 never, 1 always */
    int tune_mark_quick = 1; /* rt_tuning key 18: quick reject in k_halo_mark */
    int tune_mark_window = 1; /* rt_tuning key 19 (r04): k_halo_mark collects a workgroup's marks in LDS first */
    unsigned long long* d_wire = nullptr; /* rt_wire_delay: GPU clock stamps */
    int wall_khz = 100000;
    uint32_t* d_tile_perm[4] = {nullptr, nullptr, nullptr, nullptr}; /* rt_exp_tile_perm (experiments library): dispatch order of a tracing kernel */
    size_t tile_perm_n[4] = {0, 0, 0, 0};
    unsigned long long* d_wave_clock = nullptr; /* rt_exp_wave_clock (experiments library): two words per wavefront of one kernel */
    size_t wave_clock_words = 0;
    int wave_clock_kernel = -1, wave_clock_pass = 0;
    int tune_fuse_raycast = -1; /* rt_tuning key 25 (r05): stage 0 as ONE launch (primary ray, then candidates + temporal merge): -1 auto */
    int tune_half_raycast = 0; /* rt_tuning key 24 (r05, experiments build): half-density raycast with helper lanes */
    int tune_fuse_final = -1; /* rt_tuning key 23 (r05): last spatial pass + resolve in one kernel: -1 auto, 0 never, 1 always, 2 = A/B without the pass's stores */
    bool spatial_unbiased = false; /* rt_spatial_unbiased: the spatial passes normalise by 1/Z (k_spatial_unbiased) */
    int tune_spec_free = -1; /* rt_tuning key 22 (r05): the look-ahead stage 0 free of the main stream and of the latest resolve: -1 auto = strips */
    int tune_mark_split = 0; /* rt_tuning key 26 (r06): k_halo_mark as one workgroup per (tile, pass) instead of per tile. Measured, no gain: rank 4 of
                                8, WIRE_MODEL 0.3286 / 0.3314 (on) against 0.3310 / 0.3293 ms (off) at 1080p, 0.915 / 0.910 against 0.923 / 0.916 at 4K,
                                MIRROR 0.292 / 0.288 against 0.287 / 0.283 and 0.810 / 0.816 against 0.811 / 0.808 (profiles/r06_mark_split_ab.txt):
                                the marks are not on the frame's critical chain and their total work is the same. Default off. */
    int tune_mark_cache = 1; /* rt_tuning key 21 (r05): the shaded-bit rows of the halo marks are built once per epoch */
    uint64_t mark_bits_epoch = 0; /* epoch d_mark_bits was built under (0: not cached) */
    hipEvent_t ev_mark_bits = nullptr;
    bool mark_bits_event_valid = false, mark_bits_rebuilt = false;
    int tune_fuse_tonemap = 1; /* rt_tuning key 20 (r05): the staged frame's resolve kernel tone-maps its own pixel */
    HaloFuse fuse = {};        /* rt_halo_fuse_set: halo lists read / written by the running stage's spatial pass itself */
    uint64_t res_epoch = 1; /* bumped by every call that writes a reservoir buffer outside the staged frame */
    /* the staged frame in flight: the reservoir buffers' roles (frame_roles.h) and what its stages hand each other */
    struct : FrameRoles
    {
        int stage = 0, number = 0;
        bool clear = false;
        bool gen_taken = false;   /* stage 0 took its candidates from the look-ahead: no generate launch of its own */
        bool final_fused = false; /* the running frame's last pass has resolved its rows */
        uint32_t tag = 0;         /* own-visibility tag of the frame's launches (ownv_serial above) */
        bool one_launch = false;  /* the last staged frame's stage 0 on the main stream traced its primary rays in the candidates' launch */
    } frame;
    uint64_t halo_flags_epoch[2] = {0, 0}; /* epoch at which the neighbour's shaded flags were unpacked (valid while it is the current one) */
    unsigned long long* d_counter = nullptr;
    float4* d_paths[2] = {nullptr, nullptr}; /* wavefront path tracer: live-path lists (64 B per path) */
    unsigned long long* d_pt_counters = nullptr;
    int pt_wavefront = 2; /* rt_tuning key 6: 0 one launch per frame, 1 wavefront, 2 auto (wavefront for 09_ris) */
    /* rt_indirect (r36, indirect.h): bounces of the pass rt_frame runs between resolve and tone mapping (0 = off);
     * d_ind_counters: 64 words (frame_kernels.h, k_indirect), ind_bounces: the last pass's; ind_ev: its device time while rt_timing_enable is on */
    int indirect = 0, ind_bounces = 0;
    unsigned long long* d_ind_counters = nullptr;
    hipEvent_t ind_ev[2] = {nullptr, nullptr};
    bool ind_timed = false;
    int tune_ao_layout = 0; /* rt_tuning key 27: ambient occlusion (rt_path_trace 4 / 6) 0 pixel-major, 1 ray-major (frame_kernels.h k_ao) */
    /* rt_denoise (denoise_kernels.h), allocated at the first call: the guide (rt_visibility records, {x, f}, {n, word}), the colour
     * records {e, var} of the two ping-pong sides, the HDR output; per-kernel events while rt_timing_enable is on */
    float4 *d_dn_vis = nullptr, *d_dn_gx = nullptr, *d_dn_gn = nullptr, *d_dn_col[2] = {nullptr, nullptr}, *d_dn_hdr = nullptr;
    bool dn_valid = false, dn_timed = false;
    int tune_dn_layout = DN_LAYOUT_DEFAULT; /* rt_tuning key 28: a-trous levels 0 = per-lane gathers, 1 = residue lattice in LDS */
    hipEvent_t dn_ev[5] = {};
    /* rt_denoise_temporal's history, allocated at the first call: guides {x, f} / {n, word} and moments {mu1, mu2, h, 0} of the
     * current [dt_cur] and the previous [1 - dt_cur] call, the colour history (level 1's output), the previous RayGenerator;
     * dt_valid: a history exists (rt_scene_set and rt_denoise_temporal_reset clear it). It scratches d_dn_col / d_dn_vis / d_dn_hdr. */
    float4 *d_dt_gx[2] = {nullptr, nullptr}, *d_dt_gn[2] = {nullptr, nullptr}, *d_dt_mom[2] = {nullptr, nullptr}, *d_dt_col = nullptr;
    HistoryTag dt_tag;                    /* the camera, geometry generation and eye the history was written under */
    bool dt_followed = false;             /* the last rt_denoise_temporal call was a followed call */
    int dt_cur = 0;
    bool dt_valid = false, dt_timed = false;
    hipEvent_t dt_ev[6] = {};
    /* rt_denoise_temporal_antilag (denoise_antilag.h): the toggle and its parameters; al_adapted: the last rt_denoise_temporal call was
     * an adapted call; al_ev: the start of k_denoise_antilag in a timed adapted call (its end is dt_ev[2]) */
    bool al_on = false, al_adapted = false, al_timed = false;
    rt_denoise_antilag_params al_params = {4, 0.2f, 0.8f, 0.05f};
    hipEvent_t al_ev = nullptr;
    void* d_stage = nullptr;
    size_t stage_bytes = 0;

    rt_options opt;
    rt_raygen rg;
    float eye[3] = {0, 0, 0};
    bool has_camera = false, has_scene = false;
    float cam_eye[3] = {8.0f, 8.0f, 8.0f}, cam_at[3] = {0.0f, 0.0f, 0.0f}, cam_fovy = 0.78539816339f; /* misc.hpp:217-218 */
    bool cam_updated = false;
    /* bumped by everything that can change the G-buffer or the spatial pass's neighbour choice (camera,
     * options, scene, rows, uploads): the strip driver keys its cached halo plans on it */
    uint64_t epoch = 1;

    bool timing = false;
    hipEvent_t ev[10] = {};
    bool ev_created = false;
    float last_ms[9] = {};
    bool last_valid = false;
};

#define RT_CHECK_CTX(ctx) \
    if (!(ctx)) return RT_ERR_ARG;
#define RT_FAIL(ctx, code, ...)                       \
    do                                                \
    {                                                 \
        char _b[512];                                 \
        snprintf(_b, sizeof(_b), __VA_ARGS__);        \
        (ctx)->err = _b;                              \
        return (code);                                \
    } while (0)
#define RT_HIP(ctx, call)                                                                      \
    do                                                                                         \
    {                                                                                          \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) RT_FAIL(ctx, RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); \
    } while (0)

static int stream_priority(const char* env, int dflt);
static rt_options default_options()
{
    rt_options o;
    memset(&o, 0, sizeof(o));
    o.accumulate = 0; o.max_depth = 6;
    o.ris_sample_count = 32; o.rejection_heuristics_threshold = 0.2f;
    o.use_temporal_resampling = 0; o.use_spatial_resampling = 0;
    o.spatial_resampling_sample_count = 5; o.spatial_resampling_radius = 30.0f;
    o.spatial_resampling_passes = 3; o.use_shadowed_target_function = 0; o.use_visibility_reuse = 1;
    return o;
}

/* Where and over what a launch goes. Built by whoever decides it (an entry point, a stage run, the look-ahead stage 0) and handed
 * down by reference: the launch helpers take the stream, the rows, the tag and the G-buffer set from here and from nowhere else. */
struct Launch
{
    hipStream_t stream;
    int row0, row1, rowb0, rowb1; /* storage rows [row0,row1), and an optional second range of the same launches (rowb0 >= rowb1: none) */
    uint32_t tag;                 /* own-visibility tag (rt_device.h): the staged frame's, 0 for the per-kernel entry points */
    bool timed;                   /* rt_timing's per-kernel events belong to this lane */
    float4 *vis, *g0, *g1;        /* G-buffer set */
};
/* the context's current stream, all owned rows, the current G-buffer set: what a per-kernel entry point launches */
static Launch whole_launch(const rt_ctx* c) { return Launch{c->stream, c->row_begin, c->row_end, 0, 0, 0u, c->timing, c->gbuf.vis, c->gbuf.g0, c->gbuf.g1}; }
/* the context owns the whole image (not a strip of it) / the launch covers all rows the context owns, in one range */
static bool whole_frame(const rt_ctx* c) { return c->row_begin == 0 && c->row_end == c->H; }
static bool covers_owned_rows(const rt_ctx* c, const Launch& L) { return L.row0 == c->row_begin && L.row1 == c->row_end && L.rowb1 <= L.rowb0; }
/* the look-ahead is no longer good: the next staged frame runs its own stage 0 (ahead.gen_valid is read under ahead.valid only) */
static void drop_look_ahead(rt_ctx* c) { c->ahead.valid = false; c->ahead.gen_valid = false; }

static f3 f3_of(const float v[3]) { return F3(v[0], v[1], v[2]); }
/* a RayGenerator record as the kernels' three vectors */
static void unpack_camera(const rt_raygen& q, f3& origin, f3& right, f3& up) { origin = f3_of(q.origin); right = f3_of(q.right); up = f3_of(q.up); }

enum { K_RAYCAST = 0, K_GENERATE = 1, K_SPATIAL = 2, K_RESOLVE = 3, K_OTHER = 4 };
static FrameParams make_params(const rt_ctx* c, const Launch& L, int frame, int pass, int kernel = K_OTHER)
{
    FrameParams P;
    P.W = c->W; P.H = c->H;
    P.row0 = L.row0; P.row1 = L.row1;
    P.rowb0 = L.rowb0; P.rowb1 = L.rowb1;
    P.lrow0 = c->lrow0; P.lrows = c->lrows;
    P.frame = frame; P.pass = pass;
    P.eye = f3_of(c->eye);
    unpack_camera(c->rg, P.rg_origin, P.rg_right, P.rg_up);
    P.n_lights = c->n_lights;
    P.accumulate = c->opt.accumulate; P.ris_sample_count = c->opt.ris_sample_count;
    P.use_temporal = c->opt.use_temporal_resampling; P.use_spatial = c->opt.use_spatial_resampling;
    P.spatial_count = c->opt.spatial_resampling_sample_count; P.vis_reuse = c->opt.use_visibility_reuse;
    P.spatial_radius = c->opt.spatial_resampling_radius;
    {
        /* auto. r01-r04 gave XCD k ONE band of tile rows in every kernel (order inside the band: r04, profiles/r04_strip_tile_modes.txt).
         * The tracing kernels' cost per tile follows the scene (sky rows, brick rows ...), so the launch ended with the dearest
         * band's XCD while the others idled: r05 interleaves their tiles over the XCDs — whole frames by tile rows (2), strips
         * tile by tile (4: balanced for any height) — raycast -14 %, generate_candidate -9 %, resolve -12 % of a whole frame; an
         * 8-rank 4K strip -7 % with its spatial launches interleaved too (a 1080p one +-0). The whole frame's spatial pass keeps
         * its bands: its neighbour window has to stay in one XCD's L2 (interleaved: 0.132 -> 0.199 ms), and cutting the bands by
         * cost instead of height gains nothing (profiles/r05_spatial_band_cuts.txt). */
        const bool whole = whole_frame(c);
        /* the shadowed-target pass traces up to six rays per pixel: a tracing kernel first (runs of 16 tiles per XCD: 4.67 -> 3.83 ms
         * per frame; interleaved tile rows 3.91) */
        const int spatial = c->opt.use_shadowed_target_function ? 7 : (whole || c->row_end - c->row_begin >= 400 ? 1 : 4);
        /* interleaved tile rows give an XCD ceil(tile rows / 8) of them: within 2 % of an eighth for 1080p (135) and 4K (270), not
         * for 1280 x 720 (90 tile rows: 12 against 11.25) — runs of 16 tiles then (balanced for any shape; equal at 1080p) */
        const int tile_rows = (c->row_end - c->row_begin + 7) / 8;
        const int traced = !whole ? 4 : (50 * ((tile_rows + 7) / 8) * 8 <= 51 * tile_rows ? 2 : 7);
        const int autom = kernel == K_SPATIAL ? spatial : (kernel == K_OTHER ? 0 : traced);
        P.tile_mode = c->tune_tile_mode[kernel] >= 0 ? c->tune_tile_mode[kernel] : autom;
    }
    P.ownv_tag = L.tag;
    P.pick_mode = c->pick_mode;
    P.stats = c->walk_on ? c->d_walk : nullptr;
    P.prev_origin = P.rg_origin; P.prev_right = P.rg_right; P.prev_up = P.rg_up; /* history_camera sets the history buffer's where it differs */
    P.eye_prev = P.eye; P.motion_lo = 0u; P.motion_hi = 0u; P.tv_prev = nullptr; P.motion_vis = nullptr; P.motion_same_camera = 1; /* history_motion */
#ifdef RT_EXPERIMENTS
    P.wave_clock = c->d_wave_clock && kernel == c->wave_clock_kernel && (kernel != K_SPATIAL || pass == c->wave_clock_pass) ? c->d_wave_clock : nullptr;
    /* whole launches over the context's own rows only (the grid the permutation was checked against) */
    P.tile_perm = (kernel == K_RAYCAST || kernel == K_GENERATE || kernel == K_RESOLVE) && covers_owned_rows(c, L) ? c->d_tile_perm[kernel] : nullptr;
#endif
    return P;
}
/* the reservoir buffer `phys` is written under the current camera and generation; its shaded bits belong to G-buffer `gserial` */
static void tag_reservoir(rt_ctx* c, int phys, uint64_t gserial)
{
    c->res_tag[phys].write(c->rg, c->moved.geo_gen, c->eye, gserial);
    c->moved.tagged(FOLLOW_RESTIR);
}
static void tag_reservoir(rt_ctx* c, int phys) { tag_reservoir(c, phys, c->gbuf.serial); }
/* rt_temporal_reprojection: does a temporal merge that reads buffer `prev_phys` as its history gather by reprojection? Only with
 * the mode on and a buffer whose 36 bytes of RayGenerator differ from the current ones (then P carries them); an untagged buffer
 * and a camera that stands still launch what they launched before the mode existed. */
static bool history_camera(const rt_ctx* c, int prev_phys, FrameParams& P)
{
    if (!c->reproject || !c->opt.use_temporal_resampling || !c->res_tag[prev_phys].has) return false;
    const rt_raygen& q = c->res_tag[prev_phys].rg;
    if (tr_same_camera(q.origin, c->rg.origin)) return false; /* origin, right, up: 9 contiguous floats */
    unpack_camera(q, P.prev_origin, P.prev_right, P.prev_up);
    return true;
}
/* rt_temporal_motion: is a temporal merge that reads buffer `prev_phys` as its history a motion launch? Both toggles on, and a buffer
 * of exactly the generation d_tv_prev describes, which is not the current one; then P carries the previous camera (also where its
 * bytes are the current one's), the previous eye, the moved range and the previous vertices. An older history, or one of the
 * current generation, is history_camera's. `vis`: the Visibility buffer of the launch's rows. */
static bool history_motion(const rt_ctx* c, int prev_phys, FrameParams& P, const float4* vis)
{
    const HistoryTag& t = c->res_tag[prev_phys];
    if (!c->reproject || !c->opt.use_temporal_resampling || !c->moved.follows(FOLLOW_RESTIR, t)) return false;
    P.motion_same_camera = tr_same_camera(t.rg.origin, c->rg.origin) ? 1 : 0;
    unpack_camera(t.rg, P.prev_origin, P.prev_right, P.prev_up);
    P.eye_prev = f3_of(t.eye);
    P.motion_lo = c->moved.lo; P.motion_hi = c->moved.hi;
    P.tv_prev = c->d_tv_prev;
    P.motion_vis = vis;
    return true;
}
static bool scene_has_vertices(const rt_ctx* c) { return c->d_tv && c->n_tris > 0; }
/* the device half of MovedGeometry's "free" and "free and copy": d_tv_prev := nothing, or d_tv, all of it (the first of the two
 * toggles going on, the last going off, or a new scene while either is on) */
static int kept_vertices_replace(rt_ctx* c, bool copy)
{
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    if (!copy) return RT_OK;
    RT_HIP(c, hipMalloc(&c->d_tv_prev, (size_t)c->n_tris * 48));
    RT_HIP(c, hipMemcpyAsync(c->d_tv_prev, c->d_tv, (size_t)c->n_tris * 48, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}
/* what a changed toggle asks for (KeptAction): launches in flight may read d_tv_prev, so the stream drains first */
static int kept_vertices_toggled(rt_ctx* c, KeptAction a)
{
    if (a == KEPT_NOTHING) return RT_OK;
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    return kept_vertices_replace(c, a == KEPT_DRAIN_FREE_COPY);
}
static_assert(sizeof(rt_raygen) == 36 && offsetof(rt_raygen, right) == 12 && offsetof(rt_raygen, up) == 24, "tr_same_camera reads 9 contiguous floats");
static uint32_t next_ownv_tag(rt_ctx* c)
{
    c->ownv_serial = (c->ownv_serial + 1u) & 0x3fffffffu;
    if (c->ownv_serial == 0u) c->ownv_serial = 1u;
    return c->ownv_serial;
}
static SceneView make_scene(const rt_ctx* c)
{
    SceneView S;
    S.bvh.nodes = c->d_nodes; S.bvh.tv = c->d_tv; S.bvh.n_tris = c->n_tris;
    S.wide.rec = c->d_wide; S.wide.n_tris = c->n_tris; S.wide.n_rec = c->n_wide;
    S.trimat = c->d_trimat; S.lights = c->d_lights; S.light_ke = c->d_light_ke;
    S.light_alias = nullptr;
    return S;
}
static size_t local_pixels(const rt_ctx* c) { return (size_t)c->W * (size_t)c->lrows; }

/* for the tables of rt_trace_mode and rt_tuning at the end of the file (templates cannot live inside extern "C") */
template <class Row, int N> static constexpr bool rows_in_order(const Row (&rows)[N], int count, int Row::*id)
{
    if (N != count) return false;
    for (int i = 0; i < N; ++i)
        if (rows[i].*id != i) return false;
    return true;
}
template <int LO, int HI> static bool within(int v) { return v >= LO && v <= HI; }

extern "C" {

int rt_create(int device, int width, int height, int row_begin, int row_end, int halo, rt_ctx** out)
{
    if (!out || width <= 0 || height <= 0 || row_begin < 0 || row_end > height || row_begin >= row_end || halo < 0)
        return RT_ERR_ARG;
    /* five streams of a context want a hardware queue each (see below): the HOST exports GPU_MAX_HW_QUEUES=8 before its first
     * HIP call (the Python package, bench.py and restir_app do). The library itself does not touch the
     * environment: setenv is not safe beside the host's other threads and has no effect once HIP is initialised. */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) return RT_ERR_NO_DEVICE;
    rt_ctx* c = new rt_ctx();
    *out = c;
    c->device = device; c->W = width; c->H = height;
    c->row_begin = row_begin; c->row_end = row_end; c->halo = halo;
    c->lrow0 = row_begin - halo < 0 ? 0 : row_begin - halo;
    const int lend = row_end + halo > height ? height : row_end + halo;
    c->lrows = lend - c->lrow0;
    /* the cooperative record fetches address a reservoir buffer by 32-bit byte offsets (frame_kernels.h, wave_gather_records_at) */
    if ((size_t)c->lrows * (size_t)width > ((size_t)1 << 26)) { delete c; *out = nullptr; return RT_ERR_UNSUPPORTED; }
    c->opt = default_options();
    memset(&c->rg, 0, sizeof(c->rg));
    RT_HIP(c, hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cus = prop.multiProcessorCount;
    }
    /* All streams of the context are created here, in a fixed order: HIP maps streams onto a small pool of hardware queues
     * (GPU_MAX_HW_QUEUES, 4 unless the environment says otherwise) and hands a new stream the least-used one, so streams
     * created lazily, after a host has destroyed and re-created contexts, can land on the queue of the very stream they are
     * meant to run beside (measured: the pipelined stage 0 on the main stream's queue, 0.39 -> 0.51 ms per frame at 1080p
     * in 8 strips, profiles/r03_hw_queue_mapping.txt). Order of importance: main, pipelined stage 0, tail, second lane. */
    RT_HIP(c, hipStreamCreateWithPriority(&c->own_stream, hipStreamNonBlocking, stream_priority("RT_MAIN_PRIORITY", 0)));
    RT_HIP(c, hipStreamCreateWithPriority(&c->ahead.stream, hipStreamNonBlocking, stream_priority("RT_SPEC_PRIORITY", 0)));
    RT_HIP(c, hipStreamCreateWithPriority(&c->tail.stream, hipStreamNonBlocking, stream_priority("RT_TAIL_PRIORITY", 0)));
    /* default priority: with the lowest priority the lane was starved in some exchanges (A/B in DESIGN.md §7) */
    RT_HIP(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
    RT_HIP(c, hipEventCreateWithFlags(&c->ahead.ev_go, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ahead.ev_done, hipEventDisableTiming));
    for (auto& es : c->ahead.ev_t) for (auto& e : es) RT_HIP(c, hipEventCreate(&e));
    RT_HIP(c, hipEventCreateWithFlags(&c->tail.ev_go, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->tail.ev, hipEventDisableTiming));
    for (auto& e : c->tail.ev_resolved) RT_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_aux, hipEventDisableTiming));
    RT_HIP(c, hipEventCreateWithFlags(&c->ev_mark_bits, hipEventDisableTiming));
    c->stream = c->own_stream;
    const size_t n = local_pixels(c);
    RT_HIP(c, hipMalloc(&c->gbuf.vis, n * 16));
    RT_HIP(c, hipMalloc(&c->gbuf.g0, n * 16));
    RT_HIP(c, hipMalloc(&c->gbuf.g1, n * 16));
    RT_HIP(c, hipMalloc(&c->d_accum, n * 16));
    RT_HIP(c, hipMalloc(&c->d_pixels, n * 4));
    for (int k = 0; k < 3; ++k)
    {
        RT_HIP(c, hipMalloc(&c->d_rec[k], n * 64));
        RT_HIP(c, hipMalloc(&c->d_rad[k], n * 16));
        /* temporal history is defined as Reservoir{} before frame 1 */
        RT_HIP(c, hipMemsetAsync(c->d_rec[k], 0, n * 64, c->stream));
        RT_HIP(c, hipMemsetAsync(c->d_rad[k], 0, n * 16, c->stream));
    }
    RT_HIP(c, hipMemsetAsync(c->gbuf.vis, 0, n * 16, c->stream));
    RT_HIP(c, hipMemsetAsync(c->gbuf.g0, 0, n * 16, c->stream));
    RT_HIP(c, hipMemsetAsync(c->gbuf.g1, 0, n * 16, c->stream));
    RT_HIP(c, hipMemsetAsync(c->d_accum, 0, n * 16, c->stream));
    RT_HIP(c, hipMemsetAsync(c->d_pixels, 0, n * 4, c->stream));
    c->gbuf.set[0][0] = c->gbuf.vis; c->gbuf.set[0][1] = c->gbuf.g0; c->gbuf.set[0][2] = c->gbuf.g1;
    RT_HIP(c, hipMalloc(&c->d_counter, 8));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

/* rt_light_grid's device tables */
static void free_light_grid_tables(rt_ctx* c)
{
    hipFree(c->d_grid_cells); hipFree(c->d_grid_cell_prob); hipFree(c->d_grid_runs); hipFree(c->d_grid_run_slots); hipFree(c->d_grid_cluster_of);
    hipFree(c->d_lights_grid); hipFree(c->d_light_ke_grid);
    c->d_grid_cells = nullptr; c->d_grid_cell_prob = nullptr; c->d_grid_runs = nullptr; c->d_grid_run_slots = nullptr; c->d_grid_cluster_of = nullptr;
    c->d_lights_grid = nullptr; c->d_light_ke_grid = nullptr;
    c->grid_built = false;
}
/* ... and the host state with them; the request (grid_cells, grid_clusters) stays */
static void free_light_grid(rt_ctx* c)
{
    free_light_grid_tables(c);
    c->h_grid = LightGrid();
    std::vector<float>().swap(c->h_grid_tris);
    c->grid_built = false;
}
static void free_scene(rt_ctx* c)
{
    free_light_grid(c);
    hipFree(c->d_tris); hipFree(c->d_tv); hipFree(c->d_nodes); hipFree(c->d_trimat); hipFree(c->d_lights); hipFree(c->d_light_ke); hipFree(c->d_wide);
    hipFree(c->d_lights_power); hipFree(c->d_alias);
    c->d_lights_power = nullptr; c->d_alias = nullptr;
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    c->h_light_w.clear(); c->h_alias.clear(); c->h_alias_K.clear(); c->alias_ok = false;
    hipFree(c->d_light_ids); hipFree(c->d_refit_list); hipFree(c->d_refit_box); hipFree(c->d_refit_bounds);
    c->d_light_ids = nullptr; c->d_refit_list = nullptr; c->d_refit_box = nullptr; c->d_refit_bounds = nullptr;
    if (c->d_frag_uv) hipFree(c->d_frag_uv); /* only a scene that was updated has them: a static scene's rt_scene_set makes no call for them */
    if (c->d_frag_n) hipFree(c->d_frag_n);
    c->d_frag_uv = nullptr; c->d_frag_n = nullptr; c->n_frags = 0; c->frag_pending = false; c->cost_at_build = -1.0;
    c->h_lights.clear(); c->refit_off.clear();
    c->bin_stale = false;
    c->d_light_ke = nullptr;
    c->d_wide = nullptr;
    c->d_tris = nullptr; c->d_tv = nullptr; c->d_nodes = nullptr; c->d_trimat = nullptr; c->d_lights = nullptr;
    c->has_scene = false;
}

int rt_destroy(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    hipSetDevice(c->device);
    if (c->stream && c->stream != c->own_stream) hipStreamSynchronize(c->stream);
    if (c->own_stream) hipStreamSynchronize(c->own_stream);
    if (c->ahead.stream) hipStreamSynchronize(c->ahead.stream); /* may still read the scene: before free_scene */
    if (c->tail.stream) { hipStreamSynchronize(c->tail.stream); hipStreamDestroy(c->tail.stream); }
    if (c->tail.ev_go) hipEventDestroy(c->tail.ev_go);
    if (c->tail.ev) hipEventDestroy(c->tail.ev);
    for (auto& e : c->tail.ev_resolved) if (e) hipEventDestroy(e);
    drop_look_ahead(c);
    if (c->aux_stream) { hipStreamSynchronize(c->aux_stream); hipStreamDestroy(c->aux_stream); }
    if (c->ev_stage) hipEventDestroy(c->ev_stage);
    if (c->ev_aux) hipEventDestroy(c->ev_aux);
    if (c->ev_mark_bits) hipEventDestroy(c->ev_mark_bits);
    free_scene(c);
    if (c->ahead.stream) { hipStreamSynchronize(c->ahead.stream); hipStreamDestroy(c->ahead.stream); }
    if (c->ahead.ev_go) hipEventDestroy(c->ahead.ev_go);
    if (c->ahead.ev_done) hipEventDestroy(c->ahead.ev_done);
    for (auto& es : c->ahead.ev_t) for (auto& e : es) if (e) hipEventDestroy(e);
    for (auto& gs : c->gbuf.set) for (auto& p : gs) hipFree(p);
    hipFree(c->d_accum); hipFree(c->d_pixels);
    for (int k = 0; k < 5; ++k) { hipFree(c->d_rec[k]); hipFree(c->d_rad[k]); }
    hipFree(c->d_shaded_bits); hipFree(c->d_mark_bits);
    hipFree(c->d_visq[0]); hipFree(c->d_visq[1]); hipFree(c->d_visq_count);
    if (c->h_visq_count) hipHostFree(c->h_visq_count);
    hipFree(c->d_hints);
    hipFree(c->d_walk); hipFree(c->d_wire); hipFree(c->d_wave_clock);
    for (auto& p : c->d_tile_perm) hipFree(p);
    hipFree(c->d_dn_vis); hipFree(c->d_dn_gx); hipFree(c->d_dn_gn); hipFree(c->d_dn_col[0]); hipFree(c->d_dn_col[1]); hipFree(c->d_dn_hdr);
    for (auto& e : c->dn_ev) if (e) hipEventDestroy(e);
    for (int k = 0; k < 2; ++k) { hipFree(c->d_dt_gx[k]); hipFree(c->d_dt_gn[k]); hipFree(c->d_dt_mom[k]); }
    hipFree(c->d_dt_col);
    for (auto& e : c->dt_ev) if (e) hipEventDestroy(e);
    if (c->al_ev) hipEventDestroy(c->al_ev);
    hipFree(c->d_lf_words); hipFree(c->d_lf_stage);
    for (hipEvent_t e : c->lf_ev) if (e) hipEventDestroy(e);
    hipFree(c->d_ind_counters);
    for (hipEvent_t e : c->ind_ev) if (e) hipEventDestroy(e);
    hipFree(c->d_counter); hipFree(c->d_stage); hipFree(c->d_paths[0]); hipFree(c->d_paths[1]); hipFree(c->d_pt_counters);
    if (c->ev_created) for (auto& e : c->ev) hipEventDestroy(e);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
    return RT_OK;
}

const char* rt_last_error(rt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int rt_set_stream(rt_ctx* c, void* s)
{
    RT_CHECK_CTX(c);
    /* exactly the caller's stream; NULL is HIP's null (default) stream, which is what
     * torch.cuda.current_stream() is unless the caller entered a stream context */
    c->stream = (hipStream_t)s;
    return RT_OK;
}
int rt_set_stream_own(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    c->stream = c->own_stream;
    return RT_OK;
}
int rt_sync(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->ahead.stream) RT_HIP(c, hipStreamSynchronize(c->ahead.stream)); /* the next frame's raycast is work of this call too */
    if (c->tail.stream) RT_HIP(c, hipStreamSynchronize(c->tail.stream));
    c->tail.pending_main = false;
    return RT_OK;
}

static int ensure_stage(rt_ctx* c, size_t bytes)
{
    if (c->stage_bytes >= bytes) return RT_OK;
    if (c->d_stage) { RT_HIP(c, hipStreamSynchronize(c->stream)); hipFree(c->d_stage); c->d_stage = nullptr; }
    RT_HIP(c, hipMalloc(&c->d_stage, bytes));
    c->stage_bytes = bytes;
    return RT_OK;
}

static int build_wide(rt_ctx* c, const rt_triangle* tris, int n_refs)
{
    const size_t n_bin = (size_t)(n_refs > 1 ? n_refs - 1 : 1);
    std::vector<BvhNode> bin(n_bin);
    RT_HIP(c, hipMemcpyAsync(bin.data(), c->d_nodes, n_bin * sizeof(BvhNode), hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<WideRec> recs;
    c->wide_height = collapse_wide(bin, tris, recs, c->bvh_bfs_records);
    if (RT_WIDE_TOTAL_STACK >= 64 && 3 * c->wide_height + 1 > WIDE_LDS_STACK + WIDE_OVF_STACK)
        RT_FAIL(c, RT_ERR_BVH_DEPTH, "wide BVH height %d exceeds the traversal stack (%d entries)", c->wide_height,
                WIDE_LDS_STACK + WIDE_OVF_STACK);
    c->n_wide = (int)recs.size();
    RT_HIP(c, hipMalloc(&c->d_wide, recs.size() * sizeof(WideRec)));
    RT_HIP(c, hipMemcpyAsync(c->d_wide, recs.data(), recs.size() * sizeof(WideRec), hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

/* The whole build on the device (bvh_build_device.h): pre-split, Morton sort, PLOC hierarchy, wide collapse.
 * The host only reads counters back. */
#ifndef RT_PLOC_TOP
#define RT_PLOC_TOP 8192 /* clusters left when the host builds the top of the tree (builder 2): 2048 / 8192 / 32768 -> build 10.4 / 13.3 / 25.3 ms, frame +3.5 / +1.5 / +0.5 % against the host SAH tree */
#endif
struct FragCount64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; } };
static int build_bvh_device(rt_ctx* c, int n_tris)
{
    hipStream_t st = c->stream;
    std::vector<void*> tmp; /* device scratch, freed on every exit */
    auto cleanup = [&]() { for (void* p : tmp) hipFree(p); tmp.clear(); };
    auto dalloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr; tmp.push_back(p); return p; };
#define BD_FAIL(code, ...) do { char _b[256]; snprintf(_b, sizeof(_b), __VA_ARGS__); c->err = _b; cleanup(); return (code); } while (0)
#define BD_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) BD_FAIL(RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(_e)); } while (0)
#define BD_PTR(p) do { if (!(p)) BD_FAIL(RT_ERR_HIP, "out of device memory in the BVH build"); } while (0)
    const int gt = (n_tris + 255) / 256;
    /* 1. extents, scene bounds, median extent */
    float* d_ext = (float*)dalloc((size_t)n_tris * 4); BD_PTR(d_ext);
    float* d_ext2 = (float*)dalloc((size_t)n_tris * 4); BD_PTR(d_ext2);
    unsigned int* d_bounds = (unsigned int*)dalloc(24); BD_PTR(d_bounds);
    const unsigned int binit[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    BD_HIP(hipMemcpyAsync(d_bounds, binit, 24, hipMemcpyHostToDevice, st));
    k_tri_extents<<<gt, 256, 0, st>>>(c->d_tris, n_tris, d_ext, d_bounds);
    BD_HIP(hipGetLastError());
    size_t tb = 0;
    BD_HIP(rocprim::radix_sort_keys(nullptr, tb, d_ext, d_ext2, (size_t)n_tris, 0, 32, st));
    void* d_t0 = dalloc(tb); BD_PTR(d_t0);
    BD_HIP(rocprim::radix_sort_keys(d_t0, tb, d_ext, d_ext2, (size_t)n_tris, 0, 32, st));
    float median = 0.0f;
    unsigned int hb[6];
    BD_HIP(hipMemcpyAsync(&median, d_ext2 + n_tris / 2, 4, hipMemcpyDeviceToHost, st));
    BD_HIP(hipMemcpyAsync(hb, d_bounds, 24, hipMemcpyDeviceToHost, st));
    BD_HIP(hipStreamSynchronize(st));
    auto dec = [](unsigned int u) -> float { const unsigned int v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; float f; memcpy(&f, &v, 4); return f; };
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = dec(hb[a]); hi[a] = dec(hb[3 + a]); }
    float ext = 0.0f;
    for (int a = 0; a < 3; ++a) ext = fmaxf(ext, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    const float pad = 4e-5f * (ext > 1.0f ? ext : 1.0f); /* as the host path: hits lie within rounding distance of the triangle */
    const float3 slo = make_float3(lo[0], lo[1], lo[2]);
    const float3 sext = make_float3(fmaxf(hi[0] - lo[0], 1e-20f), fmaxf(hi[1] - lo[1], 1e-20f), fmaxf(hi[2] - lo[2], 1e-20f));
    (void)slo; (void)sext; /* Morton keys: builder 2 (experiments build) */
    /* 2. early split clipping: count, scan, emit */
    uint32_t* d_cnt = (uint32_t*)dalloc((size_t)n_tris * 4); BD_PTR(d_cnt);
    uint32_t* d_off = (uint32_t*)dalloc((size_t)n_tris * 4); BD_PTR(d_off);
    size_t sb = 0;
    BD_HIP(rocprim::exclusive_scan(nullptr, sb, d_cnt, d_off, 0u, (size_t)n_tris, rocprim::plus<uint32_t>(), st));
    void* d_t1 = dalloc(sb); BD_PTR(d_t1);
    float L = c->bvh_split_factor > 0.0f ? c->bvh_split_factor * median : 0.0f;
    const uint64_t budget = (uint64_t)n_tris * 4 + 1024;
    /* the total in 64 bits (FragCount64): up to FRAG_MAX_PER_TRI fragments of each of more than 2^20 triangles wrap 32 */
    uint64_t* d_total = (uint64_t*)dalloc(8); BD_PTR(d_total);
    auto cnt64 = rocprim::make_transform_iterator(d_cnt, FragCount64());
    size_t rdb = 0;
    BD_HIP(rocprim::reduce(nullptr, rdb, cnt64, d_total, (uint64_t)0, (size_t)n_tris, rocprim::plus<uint64_t>(), st));
    void* d_t1b = dalloc(rdb); BD_PTR(d_t1b);
    hipError_t count_err = hipSuccess;
    uint64_t total = 0;
    L = frag_fit_length(L, budget, [&](float len) -> uint64_t {
        /* per-triangle counts at `len` and their 64-bit sum; an error ends the search (0 fits) and is reported below */
        uint64_t sum = 0;
        k_split_refs<false><<<gt, 256, 0, st>>>(c->d_tris, n_tris, len, pad, nullptr, d_cnt, nullptr, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = rocprim::reduce(d_t1b, rdb, cnt64, d_total, (uint64_t)0, (size_t)n_tris, rocprim::plus<uint64_t>(), st);
        if (e == hipSuccess) e = hipMemcpyAsync(&sum, d_total, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { count_err = e; return 0; }
        return sum;
    }, &total);
    if (count_err != hipSuccess) BD_FAIL(RT_ERR_HIP, "counting the pre-split fragments failed: %s", hipGetErrorString(count_err));
    if (total > budget || total > (uint64_t)INT32_MAX) BD_FAIL(RT_ERR_STATE, "internal: %llu pre-split references for %d triangles", (unsigned long long)total, n_tris);
    /* offsets of the accepted counts: total <= budget < 2^32, so this 32-bit scan cannot wrap */
    BD_HIP(rocprim::exclusive_scan(d_t1, sb, d_cnt, d_off, 0u, (size_t)n_tris, rocprim::plus<uint32_t>(), st));
    const int n = (int)total;
    c->n_refs = n;
    float* d_boxes = (float*)dalloc((size_t)n * 24); BD_PTR(d_boxes);
    int* d_ref_tri = (int*)dalloc((size_t)n * 4); BD_PTR(d_ref_tri);
    k_split_refs<true><<<gt, 256, 0, st>>>(c->d_tris, n_tris, L, pad, d_off, nullptr, d_boxes, d_ref_tri);
    BD_HIP(hipGetLastError());
    BD_HIP(hipMalloc(&c->d_tv, (size_t)n_tris * 48));
    k_bvh_tv<<<gt, 256, 0, st>>>(c->d_tris, n_tris, c->d_tv);
    BD_HIP(hipGetLastError());
    if (n < 2) BD_FAIL(RT_ERR_STATE, "internal: the device build needs at least two references");
    const int grid = (n + 255) / 256;
    int2* d_children = (int2*)dalloc((size_t)n * 8); BD_PTR(d_children);
    int* d_parent = (int*)dalloc((size_t)n * 4); BD_PTR(d_parent);
    float* d_node_boxes = (float*)dalloc((size_t)n * 24); BD_PTR(d_node_boxes);
    const uint32_t* d_leaf_ids = nullptr; /* leaf position -> reference, for k_bvh_emit */
    SahState* d_sah_state = nullptr;
    if (c->bvh_builder == 3)
    {
        /* 3b. top-down binned SAH on the device (bvh_build_device.h): the host enqueues levels and, from level 16 on,
         * looks every fourth level whether large nodes are left (24 bytes of counters; a balanced tree over 2^24 references
         * is done by then, deeper ones keep going up to SAH_MAX_LEVELS) */
        const int max_active = n / (SAH_SMALL + 1) + 2, max_small = n / 2 + 2;
        uint32_t* d_order[2] = {(uint32_t*)dalloc((size_t)n * 4), (uint32_t*)dalloc((size_t)n * 4)}; BD_PTR(d_order[0]); BD_PTR(d_order[1]);
        int* d_seg[2] = {(int*)dalloc((size_t)n * 4), (int*)dalloc((size_t)n * 4)}; BD_PTR(d_seg[0]); BD_PTR(d_seg[1]);
        unsigned int* d_flag = (unsigned int*)dalloc((size_t)n * 4); BD_PTR(d_flag);
        unsigned int* d_pre = (unsigned int*)dalloc((size_t)n * 4); BD_PTR(d_pre);
        SahNode* d_act[2] = {(SahNode*)dalloc((size_t)max_active * sizeof(SahNode)), (SahNode*)dalloc((size_t)max_active * sizeof(SahNode))}; BD_PTR(d_act[0]); BD_PTR(d_act[1]);
        SahSplit* d_splits = (SahSplit*)dalloc((size_t)max_active * sizeof(SahSplit)); BD_PTR(d_splits);
        const size_t bin_words = (size_t)max_active * SAH_NODE_BIN_WORDS;
        unsigned int* d_bins = (unsigned int*)dalloc(bin_words * 4); BD_PTR(d_bins);
        SahSmallRoot* d_small = (SahSmallRoot*)dalloc((size_t)max_small * sizeof(SahSmallRoot)); BD_PTR(d_small);
        d_sah_state = (SahState*)dalloc(sizeof(SahState)); BD_PTR(d_sah_state);
        size_t scan_bytes = 0;
        BD_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, d_flag, d_pre, 0u, (size_t)n, rocprim::plus<unsigned int>(), st));
        void* d_scan_tmp = dalloc(scan_bytes); BD_PTR(d_scan_tmp);
        BD_HIP(hipMemsetAsync(d_parent, 0xff, 4, st)); /* the root has no parent */
        const int big_grid = (n + SAH_BLOCK - 1) / SAH_BLOCK;
        k_sah_begin<<<1, 1, 0, st>>>(d_sah_state);
        k_sah_root_bounds<<<big_grid, SAH_BLOCK, 0, st>>>(n, d_boxes, d_order[0], d_seg[0], d_sah_state);
        k_sah_root<<<1, 1, 0, st>>>(n, d_sah_state, d_act[0], d_small);
        BD_HIP(hipGetLastError());
        constexpr int SAH_MAX_LEVELS = 4096;
        const int clear_grid = (int)std::min<size_t>((bin_words + 255) / 256, 4096);
        int levels_run = 0;
        bool large_left = n > SAH_SMALL;
        while (large_left && levels_run < SAH_MAX_LEVELS)
        {
            const int level = levels_run, r = level & 1, w = r ^ 1;
            k_sah_clear_bins<<<clear_grid, 256, 0, st>>>(level, d_sah_state, d_bins, bin_words);
            k_sah_bin<<<big_grid, SAH_BLOCK, 0, st>>>(n, level, d_sah_state, d_act[r], d_boxes, d_order[r], d_seg[r], d_bins);
            k_sah_split<<<max_active, 64, 0, st>>>(level, d_sah_state, d_act[r], d_act[w], d_bins, d_splits, d_small, d_children, d_parent, d_node_boxes, max_active, max_small);
            k_sah_medium<<<max_active, SAH_BLOCK, 0, st>>>(level, d_sah_state, d_act[r], d_act[w], d_boxes, d_order[r], d_splits, d_small, d_children, d_parent, d_node_boxes, max_active, max_small);
            k_sah_classify<<<grid, 256, 0, st>>>(n, level, d_sah_state, d_splits, d_boxes, d_order[r], d_seg[r], d_flag);
            BD_HIP(rocprim::exclusive_scan(d_scan_tmp, scan_bytes, d_flag, d_pre, 0u, (size_t)n, rocprim::plus<unsigned int>(), st));
            k_sah_scatter<<<grid, 256, 0, st>>>(n, level, d_sah_state, d_splits, d_flag, d_pre, d_order[r], d_seg[r], d_order[w], d_seg[w]);
            k_sah_next_level<<<1, 1, 0, st>>>(level, d_sah_state);
            ++levels_run;
            if (levels_run >= 16 && (levels_run & 3) == 0)
            {
                SahState probe;
                BD_HIP(hipGetLastError());
                BD_HIP(hipMemcpyAsync(&probe, d_sah_state, sizeof(probe), hipMemcpyDeviceToHost, st));
                BD_HIP(hipStreamSynchronize(st));
                large_left = probe.n_active[levels_run & 1] != 0u;
            }
        }
        BD_HIP(hipGetLastError());
        uint32_t* d_final = d_order[levels_run & 1];
        k_sah_small<<<max_small, 64, 0, st>>>(d_sah_state, d_small, d_boxes, d_final, d_children, d_parent, d_node_boxes);
        BD_HIP(hipGetLastError());
        d_leaf_ids = d_final;
    }
#ifdef RT_EXPERIMENTS
    else
    {
    /* 3. Morton order */
    uint64_t* d_keys = (uint64_t*)dalloc((size_t)n * 8); BD_PTR(d_keys);
    uint64_t* d_keys2 = (uint64_t*)dalloc((size_t)n * 8); BD_PTR(d_keys2);
    uint32_t* d_ids = (uint32_t*)dalloc((size_t)n * 4); BD_PTR(d_ids);
    uint32_t* d_ids2 = (uint32_t*)dalloc((size_t)n * 4); BD_PTR(d_ids2);
    k_bvh_keys<<<grid, 256, 0, st>>>(d_boxes, n, slo, sext, d_keys, d_ids);
    BD_HIP(hipGetLastError());
    size_t rb = 0;
    BD_HIP(rocprim::radix_sort_pairs(nullptr, rb, d_keys, d_keys2, d_ids, d_ids2, (size_t)n, 0, 64, st));
    void* d_t2 = dalloc(rb); BD_PTR(d_t2);
    BD_HIP(rocprim::radix_sort_pairs(d_t2, rb, d_keys, d_keys2, d_ids, d_ids2, (size_t)n, 0, 64, st));
    /* 4. PLOC hierarchy */
    int* d_cid[2] = {(int*)dalloc((size_t)n * 4), (int*)dalloc((size_t)n * 4)}; BD_PTR(d_cid[0]); BD_PTR(d_cid[1]);
    float* d_cbox[2] = {(float*)dalloc((size_t)n * 24), (float*)dalloc((size_t)n * 24)}; BD_PTR(d_cbox[0]); BD_PTR(d_cbox[1]);
    int* d_nn = (int*)dalloc((size_t)n * 4); BD_PTR(d_nn);
    unsigned int* d_keep = (unsigned int*)dalloc((size_t)n * 4); BD_PTR(d_keep);
    unsigned int* d_pos = (unsigned int*)dalloc((size_t)n * 4); BD_PTR(d_pos);
    PlocState* d_ps = (PlocState*)dalloc(sizeof(PlocState)); BD_PTR(d_ps);
    size_t pb = 0;
    BD_HIP(rocprim::exclusive_scan(nullptr, pb, d_keep, d_pos, 0u, (size_t)n, rocprim::plus<unsigned int>(), st));
    void* d_t3 = dalloc(pb); BD_PTR(d_t3);
    k_ploc_init<<<grid, 256, 0, st>>>(n, d_ids2, d_boxes, d_cid[0], d_cbox[0], d_ps, d_parent);
    BD_HIP(hipGetLastError());
    int cur = 0;
    bool done = n <= RT_PLOC_TOP;
    PlocState ps = {(unsigned int)n, 0u};
    for (int batch = 0; batch < 256 && !done; ++batch)
    {
        /* 12 rounds between looks at the cluster count, 2 once the top is near */
        const int rounds = ps.m > 16u * RT_PLOC_TOP ? 12 : 2;
        for (int it = 0; it < rounds; ++it)
        {
            k_ploc_nn<<<grid, 256, 0, st>>>(d_ps, d_cbox[cur], d_nn, c->ploc_radius);
            k_ploc_merge<<<grid, 256, 0, st>>>(d_ps, n, d_cid[cur], d_cbox[cur], d_nn, d_children, d_parent, d_node_boxes, d_keep);
            BD_HIP(rocprim::exclusive_scan(d_t3, pb, d_keep, d_pos, 0u, (size_t)n, rocprim::plus<unsigned int>(), st));
            k_ploc_compact<<<grid, 256, 0, st>>>(d_ps, n, d_keep, d_pos, d_cid[cur], d_cbox[cur], d_cid[cur ^ 1], d_cbox[cur ^ 1]);
            cur ^= 1;
        }
        BD_HIP(hipGetLastError());
        BD_HIP(hipMemcpyAsync(&ps, d_ps, sizeof(ps), hipMemcpyDeviceToHost, st));
        BD_HIP(hipStreamSynchronize(st));
        done = ps.m <= (unsigned int)RT_PLOC_TOP;
    }
    if (!done) BD_FAIL(RT_ERR_BVH_DEPTH, "PLOC did not converge");
    if (ps.merges + ps.m != (unsigned int)n) BD_FAIL(RT_ERR_STATE, "internal: PLOC holds %u clusters after %u merges of %d references", ps.m, ps.merges, n);
    if (ps.m > 1u)
    {
        /* The top of the tree — the levels every ray walks — by an exact top-down SAH sweep over the <= RT_PLOC_TOP
         * clusters that are left, on the host (0.2 MB down, ~2 ms of host work, 0.3 MB up): mutual-nearest-neighbour
         * merging in a +-16 window judges the last rounds poorly (frame +5.8 % against the host SAH tree, +1.5 % with
         * this, r02). Node ids 0 .. m-2 are exactly the ones PLOC has not handed out (it counts down from n-2); the
         * root is 0. */
        const int m = (int)ps.m;
        std::vector<int> h_cid((size_t)m);
        std::vector<float> h_box((size_t)m * 6);
        BD_HIP(hipMemcpyAsync(h_cid.data(), d_cid[cur], (size_t)m * 4, hipMemcpyDeviceToHost, st));
        BD_HIP(hipMemcpyAsync(h_box.data(), d_cbox[cur], (size_t)m * 24, hipMemcpyDeviceToHost, st));
        BD_HIP(hipStreamSynchronize(st));
        std::vector<int2> t_children((size_t)m - 1);
        std::vector<float> t_boxes(((size_t)m - 1) * 6);
        std::vector<int> t_parent((size_t)m - 1, -1), s_idx, s_val;
        int next_id = 0;
        auto area = [](const float* b) { const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2]; return dx * dy + dy * dz + dz * dx; };
        auto grow = [](float* b, const float* o) { for (int k = 0; k < 3; ++k) { b[k] = fminf(b[k], o[k]); b[3 + k] = fmaxf(b[3 + k], o[3 + k]); } };
        auto centroid2 = [&](int item, int ax) { return h_box[(size_t)item * 6 + ax] + h_box[(size_t)item * 6 + 3 + ax]; };
        /* exact sweep SAH with three presorted item lists (by centroid per axis) kept in step by stable partitions:
         * O(m log m) in all; a range [lo, hi) holds the same items in all three lists */
        std::vector<int> sorted[3], scratch((size_t)m);
        for (int ax = 0; ax < 3; ++ax)
        {
            sorted[ax].resize((size_t)m);
            for (int i = 0; i < m; ++i) sorted[ax][(size_t)i] = i;
            std::sort(sorted[ax].begin(), sorted[ax].end(), [&](int x, int y) {
                const float cx = centroid2(x, ax), cy = centroid2(y, ax);
                return cx < cy || (cx == cy && x < y);
            });
        }
        std::vector<unsigned char> goes_left((size_t)m);
        std::vector<float> right_area((size_t)m);
        struct Job { int lo, hi, parent, side; };
        std::vector<Job> jobs;
        jobs.push_back({0, m, -1, 0});
        while (!jobs.empty())
        {
            const Job j = jobs.back();
            jobs.pop_back();
            int ref;
            if (j.hi - j.lo == 1)
            {
                ref = h_cid[(size_t)sorted[0][(size_t)j.lo]];
                if (ref >= 0) { s_idx.push_back(ref); s_val.push_back(j.parent); }
            }
            else
            {
                const int id = next_id++;
                ref = id;
                t_parent[(size_t)id] = j.parent;
                const int cnt = j.hi - j.lo;
                float best = INFINITY;
                int best_axis = 0, best_i = cnt / 2;
                float nb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                for (int ax = 0; ax < 3; ++ax)
                {
                    const int* L = sorted[ax].data() + j.lo;
                    float rb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    for (int i = cnt - 1; i >= 1; --i) { grow(rb, &h_box[(size_t)L[i] * 6]); right_area[(size_t)i] = area(rb); }
                    float lb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    for (int i = 1; i < cnt; ++i)
                    {
                        grow(lb, &h_box[(size_t)L[i - 1] * 6]);
                        const float cost = area(lb) * (float)i + right_area[(size_t)i] * (float)(cnt - i);
                        if (cost < best) { best = cost; best_axis = ax; best_i = i; }
                    }
                    if (ax == 0) { for (int k = 0; k < 6; ++k) nb[k] = lb[k]; grow(nb, &h_box[(size_t)L[cnt - 1] * 6]); }
                }
                for (int k = 0; k < 6; ++k) t_boxes[(size_t)id * 6 + k] = nb[k];
                /* the first best_i items of the best axis go left; the other two lists follow, order preserved */
                for (int i = 0; i < cnt; ++i) goes_left[(size_t)sorted[best_axis][(size_t)(j.lo + i)]] = i < best_i ? 1 : 0;
                for (int ax = 0; ax < 3; ++ax)
                {
                    if (ax == best_axis) continue;
                    int* L = sorted[ax].data() + j.lo;
                    int nl = 0, nr = 0;
                    for (int i = 0; i < cnt; ++i)
                    {
                        if (goes_left[(size_t)L[i]]) L[nl++] = L[i];
                        else scratch[(size_t)nr++] = L[i];
                    }
                    for (int i = 0; i < nr; ++i) L[nl + i] = scratch[(size_t)i];
                }
                jobs.push_back({j.lo, j.lo + best_i, id, 0});
                jobs.push_back({j.lo + best_i, j.hi, id, 1});
            }
            if (j.parent >= 0)
            {
                if (j.side == 0) t_children[(size_t)j.parent].x = ref; else t_children[(size_t)j.parent].y = ref;
            }
        }
        if (next_id != m - 1) BD_FAIL(RT_ERR_STATE, "internal: top-level build made %d nodes for %d clusters", next_id, m);
        BD_HIP(hipMemcpyAsync(d_children, t_children.data(), ((size_t)m - 1) * 8, hipMemcpyHostToDevice, st));
        BD_HIP(hipMemcpyAsync(d_node_boxes, t_boxes.data(), ((size_t)m - 1) * 24, hipMemcpyHostToDevice, st));
        BD_HIP(hipMemcpyAsync(d_parent, t_parent.data(), ((size_t)m - 1) * 4, hipMemcpyHostToDevice, st));
        if (!s_idx.empty())
        {
            int* d_si = (int*)dalloc(s_idx.size() * 4); BD_PTR(d_si);
            int* d_sv = (int*)dalloc(s_idx.size() * 4); BD_PTR(d_sv);
            BD_HIP(hipMemcpyAsync(d_si, s_idx.data(), s_idx.size() * 4, hipMemcpyHostToDevice, st));
            BD_HIP(hipMemcpyAsync(d_sv, s_val.data(), s_idx.size() * 4, hipMemcpyHostToDevice, st));
            k_scatter_int<<<((int)s_idx.size() + 255) / 256, 256, 0, st>>>((int)s_idx.size(), d_si, d_sv, d_parent);
            BD_HIP(hipGetLastError());
        }
        BD_HIP(hipStreamSynchronize(st)); /* the host vectors go out of scope */
    }
    d_leaf_ids = d_ids2;
    } /* builder 2 */
#else
    else BD_FAIL(RT_ERR_UNSUPPORTED, "BVH builder %d is an A/B form of librestir_rt_exp.so", c->bvh_builder);
#endif
    int* d_height = (int*)dalloc(4); BD_PTR(d_height);
    BD_HIP(hipMemsetAsync(d_height, 0, 4, st));
    k_bvh_height<<<grid, 256, 0, st>>>(n, d_children, d_parent, d_height);
    BD_HIP(hipMalloc(&c->d_nodes, (size_t)(n - 1) * sizeof(BvhNode)));
    k_bvh_emit<<<grid, 256, 0, st>>>(n, d_leaf_ids, d_ref_tri, d_boxes, d_children, d_parent, d_node_boxes, c->d_nodes);
    BD_HIP(hipGetLastError());
    /* which fragment of its triangle a leaf holds, for the refit (only where something was split). The 2 (n - 1) words take
     * the place of the binary nodes' boxes (6 n floats), which k_bvh_emit was the last to read: no allocation for it */
    uint32_t* d_leaf_frag = nullptr;
    if (n > n_tris)
    {
        d_leaf_frag = (uint32_t*)d_node_boxes;
        k_leaf_frags<<<grid, 256, 0, st>>>(n, d_leaf_ids, d_ref_tri, d_off, d_cnt, d_children, d_leaf_frag);
        BD_HIP(hipGetLastError());
    }
    /* 5. wide collapse, level by level */
    const size_t rec_cap = (size_t)n * 2 + 8;
    BD_HIP(hipMalloc(&c->d_wide, rec_cap * 16 * WIDE_STRIDE));
    CollapseItem* d_q[2] = {(CollapseItem*)dalloc((size_t)n * sizeof(CollapseItem)), (CollapseItem*)dalloc((size_t)n * sizeof(CollapseItem))};
    BD_PTR(d_q[0]); BD_PTR(d_q[1]);
    CollapseState* d_cs = (CollapseState*)dalloc(sizeof(CollapseState)); BD_PTR(d_cs);
    k_collapse_init<<<1, 1, 0, st>>>(d_cs, d_q[0]);
    const int max_levels = (WIDE_LDS_STACK + WIDE_OVF_STACK - 1) / 3 + 1;
    for (int level = 0; level <= max_levels; ++level)
    {
        k_collapse_level<<<grid, 256, 0, st>>>(c->d_nodes, c->d_tris, level, d_cs, d_q[level & 1], d_q[(level + 1) & 1], (uint32_t*)c->d_wide, d_leaf_frag);
        k_collapse_swap<<<1, 1, 0, st>>>(level, d_cs);
    }
    BD_HIP(hipGetLastError());
    CollapseState cs;
    int bh = 0;
    SahState sah_final;
    memset(&sah_final, 0, sizeof(sah_final));
    BD_HIP(hipMemcpyAsync(&cs, d_cs, sizeof(cs), hipMemcpyDeviceToHost, st));
    BD_HIP(hipMemcpyAsync(&bh, d_height, 4, hipMemcpyDeviceToHost, st));
    if (d_sah_state) BD_HIP(hipMemcpyAsync(&sah_final, d_sah_state, sizeof(sah_final), hipMemcpyDeviceToHost, st));
    BD_HIP(hipStreamSynchronize(st));
    if (d_sah_state)
    {
        /* the counters that came back with the heights: every level reached the small-subtree size, no table overflowed,
         * and exactly n - 1 inner nodes were made */
        if (sah_final.n_active[0] != 0u || sah_final.n_active[1] != 0u)
            BD_FAIL(RT_ERR_BVH_DEPTH, "device SAH build: large nodes left after the enqueued levels (tree deeper than expected)");
        if (sah_final.overflow != 0u || sah_final.next_node != (unsigned int)(n - 1))
            BD_FAIL(RT_ERR_STATE, "internal: device SAH build made %u inner nodes for %d references (overflow %u)", sah_final.next_node, n, sah_final.overflow);
    }
    if (cs.count[0] != 0u || cs.count[1] != 0u || 3 * (int)cs.height + 1 > WIDE_LDS_STACK + WIDE_OVF_STACK)
        BD_FAIL(RT_ERR_BVH_DEPTH, "wide BVH height %u exceeds the traversal stack (%d entries)", cs.height, WIDE_LDS_STACK + WIDE_OVF_STACK);
    if (cs.n_rec > rec_cap) BD_FAIL(RT_ERR_STATE, "internal: %u wide records for %d references", cs.n_rec, n);
    if (bh > 62) BD_FAIL(RT_ERR_BVH_DEPTH, "binary tree height %d exceeds the 63-level trail word", bh);
    c->bvh_height = bh;
    c->n_wide = (int)cs.n_rec;
    c->wide_height = (int)cs.height;
    c->frag_pending = d_leaf_frag != nullptr;
    c->frag_L = L;
    c->frag_pad = pad;
    cleanup();
#undef BD_FAIL
#undef BD_HIP
#undef BD_PTR
    return RT_OK;
}

/* LBVH build, see bvh.h */
static int build_bvh(rt_ctx* c, const rt_triangle* tris, int n_tris)
{
    if (c->bvh_builder >= 2 && n_tris >= 2) return build_bvh_device(c, n_tris);
    hipStream_t st = c->stream;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<float> extents((size_t)n_tris);
    for (int i = 0; i < n_tris; ++i)
    {
        float tl[3] = {INFINITY, INFINITY, INFINITY}, th[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a)
            {
                const float v = tris[i].v[k][a];
                tl[a] = fminf(tl[a], v);
                th[a] = fmaxf(th[a], v);
            }
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], tl[a]); hi[a] = fmaxf(hi[a], th[a]); }
        extents[i] = fmaxf(th[0] - tl[0], fmaxf(th[1] - tl[1], th[2] - tl[2]));
    }
    float ext = 0.0f;
    for (int a = 0; a < 3; ++a) ext = fmaxf(ext, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
    /* conservative padding: the accepted hit point of core.hpp:91-136 lies within rounding
     * distance of the triangle, not exactly on it */
    const float pad = 4e-5f * (ext > 1.0f ? ext : 1.0f);
    float3 slo = make_float3(lo[0], lo[1], lo[2]);
    float3 sext = make_float3(fmaxf(hi[0] - lo[0], 1e-20f), fmaxf(hi[1] - lo[1], 1e-20f), fmaxf(hi[2] - lo[2], 1e-20f));

    /* fragment length: a few median triangle extents, relaxed until the reference count fits */
    std::vector<BvhRef> refs;
    {
        std::vector<float> e2(extents);
        std::nth_element(e2.begin(), e2.begin() + e2.size() / 2, e2.end());
        float L = c->bvh_split_factor > 0.0f ? c->bvh_split_factor * e2[e2.size() / 2] : 0.0f;
        frag_fit_length(L, (uint64_t)n_tris * 4 + 1024, [&](float len) -> uint64_t {
            split_refs(tris, n_tris, len, pad, refs);
            return (uint64_t)refs.size();
        });
    }
    const int n = (int)refs.size();
    c->n_refs = n;
#ifdef RT_EXPERIMENTS
    if (c->bvh_builder == 1 && n >= 2)
    {
        SahBuilder sb(refs);
        float rl[3], rh[3];
        sb.build(0, n, -1, 1, rl, rh);
        sb.link_siblings();
        c->bvh_height = sb.height;
        if (sb.height > 62) RT_FAIL(c, RT_ERR_BVH_DEPTH, "SAH tree height %d exceeds the 63-level trail word", sb.height);
        RT_HIP(c, hipMalloc(&c->d_tv, (size_t)n_tris * 48));
        k_bvh_tv<<<(n_tris + 255) / 256, 256, 0, st>>>(c->d_tris, n_tris, c->d_tv);
        RT_HIP(c, hipGetLastError());
        RT_HIP(c, hipMalloc(&c->d_nodes, sb.nodes.size() * sizeof(BvhNode)));
        RT_HIP(c, hipMemcpyAsync(c->d_nodes, sb.nodes.data(), sb.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice, st));
        RT_HIP(c, hipStreamSynchronize(st));
        return build_wide(c, tris, n);
    }
#endif
    std::vector<float> h_boxes((size_t)n * 6);
    std::vector<int> h_ref_tri((size_t)n);
    for (int i = 0; i < n; ++i)
    {
        for (int k = 0; k < 3; ++k) { h_boxes[6 * (size_t)i + k] = refs[i].lo[k]; h_boxes[6 * (size_t)i + 3 + k] = refs[i].hi[k]; }
        h_ref_tri[i] = refs[i].tri;
    }

    RT_HIP(c, hipMalloc(&c->d_tv, (size_t)n_tris * 48));
    RT_HIP(c, hipMalloc(&c->d_nodes, (size_t)(n > 1 ? n - 1 : 1) * sizeof(BvhNode)));
    float* d_boxes = nullptr; float* d_node_boxes = nullptr;
    uint64_t *d_keys = nullptr, *d_keys2 = nullptr;
    uint32_t *d_ids = nullptr, *d_ids2 = nullptr;
    int2* d_children = nullptr; int *d_parent_inner = nullptr, *d_parent_leaf = nullptr, *d_level = nullptr, *d_remaining = nullptr;
    int* d_ref_tri = nullptr;
    void* d_temp = nullptr;
    auto cleanup = [&]() {
        hipFree(d_boxes); hipFree(d_node_boxes); hipFree(d_keys); hipFree(d_keys2); hipFree(d_ids); hipFree(d_ids2);
        hipFree(d_children); hipFree(d_parent_inner); hipFree(d_parent_leaf); hipFree(d_level); hipFree(d_remaining);
        hipFree(d_temp); hipFree(d_ref_tri);
    };
#define BV_HIP(call)                                                                               \
    do                                                                                             \
    {                                                                                              \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
        {                                                                                          \
            char _b[512];                                                                          \
            snprintf(_b, sizeof(_b), "%s failed: %s", #call, hipGetErrorString(_e));               \
            c->err = _b; cleanup(); return RT_ERR_HIP;                                             \
        }                                                                                          \
    } while (0)
    BV_HIP(hipMalloc(&d_boxes, (size_t)n * 24));
    BV_HIP(hipMalloc(&d_ref_tri, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_node_boxes, (size_t)n * 24));
    BV_HIP(hipMalloc(&d_keys, (size_t)n * 8));
    BV_HIP(hipMalloc(&d_keys2, (size_t)n * 8));
    BV_HIP(hipMalloc(&d_ids, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_ids2, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_children, (size_t)n * 8));
    BV_HIP(hipMalloc(&d_parent_inner, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_parent_leaf, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_level, (size_t)n * 4));
    BV_HIP(hipMalloc(&d_remaining, 4));
    BV_HIP(hipMemcpyAsync(d_boxes, h_boxes.data(), (size_t)n * 24, hipMemcpyHostToDevice, st));
    BV_HIP(hipMemcpyAsync(d_ref_tri, h_ref_tri.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));

    const int grid = (n + 255) / 256;
    k_bvh_tv<<<(n_tris + 255) / 256, 256, 0, st>>>(c->d_tris, n_tris, c->d_tv);
    BV_HIP(hipGetLastError());
    k_bvh_keys<<<grid, 256, 0, st>>>(d_boxes, n, slo, sext, d_keys, d_ids);
    BV_HIP(hipGetLastError());
    size_t temp_bytes = 0;
    BV_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, d_keys, d_keys2, d_ids, d_ids2, (size_t)n, 0, 64, st));
    BV_HIP(hipMalloc(&d_temp, temp_bytes > 0 ? temp_bytes : 16));
    BV_HIP(rocprim::radix_sort_pairs(d_temp, temp_bytes, d_keys, d_keys2, d_ids, d_ids2, (size_t)n, 0, 64, st));

    if (n == 1)
    {
        /* one reference: both children are the same leaf (the second test is rejected by the tie rule) */
        BvhNode nd;
        const float* hb = h_boxes.data();
        nd.a = make_float4(hb[0], hb[1], hb[2], hb[0]);
        nd.b = make_float4(hb[3], hb[4], hb[5], hb[1]);
        nd.c = make_float4(hb[3], hb[4], hb[5], hb[2]);
        nd.d = make_int4(~h_ref_tri[0], ~h_ref_tri[0], -1, -1);
        BV_HIP(hipMemcpyAsync(c->d_nodes, &nd, sizeof(nd), hipMemcpyHostToDevice, st));
        BV_HIP(hipStreamSynchronize(st));
        c->bvh_height = 1;
        cleanup();
        return build_wide(c, tris, n);
    }

    k_bvh_hierarchy<<<grid, 256, 0, st>>>(d_keys2, n, d_children, d_parent_inner, d_parent_leaf);
    BV_HIP(hipGetLastError());
    BV_HIP(hipMemsetAsync(d_level, 0, (size_t)n * 4, st));
    int height = 0;
    for (int pass = 1; pass <= 4096; ++pass)
    {
        BV_HIP(hipMemsetAsync(d_remaining, 0, 4, st));
        k_bvh_refit_pass<<<grid, 256, 0, st>>>(n, pass, d_ids2, d_boxes, d_children, d_node_boxes, d_level, d_remaining);
        BV_HIP(hipGetLastError());
        int remaining = 0;
        BV_HIP(hipMemcpyAsync(&remaining, d_remaining, 4, hipMemcpyDeviceToHost, st));
        BV_HIP(hipStreamSynchronize(st));
        if (remaining == 0) { height = pass; break; }
    }
    if (height == 0) { c->err = "LBVH refit did not converge"; cleanup(); return RT_ERR_BVH_DEPTH; }
    c->bvh_height = height;
    if (height > 62)
    {
        char b[128];
        snprintf(b, sizeof(b), "LBVH height %d exceeds the 63-level trail word", height);
        c->err = b; cleanup();
        return RT_ERR_BVH_DEPTH;
    }
    k_bvh_emit<<<grid, 256, 0, st>>>(n, d_ids2, d_ref_tri, d_boxes, d_children, d_parent_inner, d_node_boxes, c->d_nodes);
    BV_HIP(hipGetLastError());
    BV_HIP(hipStreamSynchronize(st));
    cleanup();
#undef BV_HIP
    return build_wide(c, tris, n);
}

static float light_weight_of(const rt_triangle& t)
{
    return light_weight(F3(t.v[0][0], t.v[0][1], t.v[0][2]), F3(t.v[1][0], t.v[1][1], t.v[1][2]), F3(t.v[2][0], t.v[2][1], t.v[2][2]),
                        F3(t.emissive[0], t.emissive[1], t.emissive[2]));
}
/* The alias table of rt_light_sampling from the per-light weights `w` (host, light_alias.h), uploaded next to d_lights with the light
 * table of the realised pdf. d_ids: the light list on the device; resize: the number of lights changed. Enqueues on `st`; the host
 * arrays it copies from stay until the caller's synchronisation (they are members). */
static int build_light_alias(rt_ctx* c, std::vector<float>& w, const uint32_t* d_ids, bool resize, hipStream_t st)
{
    const uint32_t L = (uint32_t)w.size();
    if (resize || !c->d_alias)
    {
        hipFree(c->d_lights_power); hipFree(c->d_alias);
        c->d_lights_power = nullptr; c->d_alias = nullptr;
    }
    c->h_light_w.swap(w);
    c->alias_ok = alias_build(c->h_light_w.data(), L, c->h_alias, c->h_alias_K);
    if (L == 0) return RT_OK;
    if (!c->d_alias)
    {
        RT_HIP(c, hipMalloc(&c->d_alias, (size_t)L * sizeof(AliasSlot)));
        RT_HIP(c, hipMalloc(&c->d_lights_power, (size_t)L * 16 * RT_LIGHT_STRIDE));
    }
    std::vector<float> prob(L);
    for (uint32_t i = 0; i < L; ++i) prob[i] = light_select_prob(c->h_alias_K[i], L);
    float* d_prob = nullptr;
    RT_HIP(c, hipMalloc(&d_prob, (size_t)L * 4));
    hipError_t e = hipMemcpyAsync(d_prob, prob.data(), (size_t)L * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_alias, c->h_alias.data(), (size_t)L * sizeof(AliasSlot), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
    {
        k_light_table<<<((int)L + 255) / 256, 256, 0, st>>>((int)L, d_ids, c->d_tris, c->d_lights_power, c->d_light_ke, d_prob);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st); /* `prob` is host memory */
    hipFree(d_prob);
    if (e != hipSuccess) RT_FAIL(c, RT_ERR_HIP, "light alias table: %s", hipGetErrorString(e));
    return RT_OK;
}

/* The tables of rt_light_grid (host, light_grid.h) from the host copy of the scene's triangles, the light list `lights` and the kept
 * weights (after build_light_alias), uploaded with a light table and a Ke table in the runs' position order: k_light_table over the
 * permuted ids, its pdf the run's factor. Reads d_tris on `st` (behind the copies the caller enqueued there) and waits for `st`. */
static int build_light_grid(rt_ctx* c, const std::vector<uint32_t>& lights, hipStream_t st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t L = (uint32_t)lights.size();
    free_light_grid_tables(c);
    LightGrid& g = c->h_grid;
    grid_build(g, c->h_grid_tris.data(), 15, (size_t)c->n_tris, lights.data(), c->h_light_w.data(), L, c->grid_cells, c->grid_clusters);
    if (L > 0)
    {
        const size_t n = g.cell_slots();
        const uint32_t B = g.B;
        std::vector<float> cell_prob(n), run_prob(L);
        std::vector<uint32_t> ids(L);
        for (size_t k = 0; k < n; ++k) cell_prob[k] = light_select_prob(g.cell_K[k], B);
        for (uint32_t r = 0; r < B; ++r)
            for (uint32_t p = g.runs[r].start; p < g.runs[r].start + g.runs[r].n; ++p)
            {
                run_prob[p] = light_select_prob(g.run_K[p], g.runs[r].n);
                ids[p] = lights[g.perm[p]];
            }
        uint32_t* d_ids = nullptr;
        float* d_prob = nullptr;
        hipError_t e = hipMalloc(&c->d_grid_cells, n * sizeof(AliasSlot));
        if (e == hipSuccess) e = hipMalloc(&c->d_grid_cell_prob, n * 4);
        if (e == hipSuccess) e = hipMalloc(&c->d_grid_runs, (size_t)B * sizeof(GridRun));
        if (e == hipSuccess) e = hipMalloc(&c->d_grid_run_slots, (size_t)L * sizeof(AliasSlot));
        if (e == hipSuccess) e = hipMalloc(&c->d_grid_cluster_of, (size_t)L * 4);
        if (e == hipSuccess) e = hipMalloc(&c->d_lights_grid, (size_t)L * 16 * RT_LIGHT_STRIDE);
        if (e == hipSuccess) e = hipMalloc(&c->d_light_ke_grid, (size_t)L * 16);
        if (e == hipSuccess) e = hipMalloc(&d_ids, (size_t)L * 4);
        if (e == hipSuccess) e = hipMalloc(&d_prob, (size_t)L * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_grid_cells, g.cells.data(), n * sizeof(AliasSlot), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_grid_cell_prob, cell_prob.data(), n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_grid_runs, g.runs.data(), (size_t)B * sizeof(GridRun), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_grid_run_slots, g.run_slots.data(), (size_t)L * sizeof(AliasSlot), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_grid_cluster_of, g.cluster_of.data(), (size_t)L * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_ids, ids.data(), (size_t)L * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_prob, run_prob.data(), (size_t)L * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
        {
            k_light_table<<<((int)L + 255) / 256, 256, 0, st>>>((int)L, d_ids, c->d_tris, c->d_lights_grid, c->d_light_ke_grid, d_prob);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st); /* the vectors above are host memory */
        hipFree(d_ids); hipFree(d_prob);
        if (e != hipSuccess)
        {
            const std::string why = hipGetErrorString(e); /* an allocation that failed (about 100 MB at 32 cells and 256 clusters) ends here too */
            free_light_grid_tables(c);
            RT_FAIL(c, RT_ERR_HIP, "rt_light_grid: tables of %d^3 cells x %u clusters: %s", c->grid_cells, B, why.c_str());
        }
    }
    c->grid_built = true;
    c->grid_build_ms = (float)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() * 1e-3f;
    return RT_OK;
}

int rt_scene_set(rt_ctx* c, const rt_triangle* triangles, uint32_t count)
{
    RT_CHECK_CTX(c);
    if (!triangles && count) RT_FAIL(c, RT_ERR_ARG, "null triangles");
    RT_HIP(c, hipSetDevice(c->device));
    /* every stream that may still read the old scene: the caller's / own stream, the speculative next-frame raycast
     * (ahead.stream) and the second lane */
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    if (c->own_stream && c->own_stream != c->stream) RT_HIP(c, hipStreamSynchronize(c->own_stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream));
    drop_look_ahead(c);
    c->dt_valid = false; /* rt_denoise_temporal's history belongs to the old scene */
    for (HistoryTag& t : c->res_tag) t.has = false; /* ... and so do the reservoir buffers' camera tags: no reprojection into it */
    /* generations count from the new scene; free_scene frees the old kept vertices, the new ones are copied once they exist (below) */
    const bool keep_vertices = c->moved.scene_set(count > 0);
    /* the remembered occluders are indices of the old scene, which may have had more triangles (every stream is idle here) */
    if (c->d_hints) RT_HIP(c, hipMemset(c->d_hints, 0xff, local_pixels(c) * sizeof(int) * OCCLUDER_HINTS));
    const auto t_build0 = std::chrono::steady_clock::now();
    free_scene(c);
    ++c->epoch;
    const int n = (int)count;
    c->n_tris = n;
    /* light list in index order (10_restir_di.cpp:196-205) */
    std::vector<uint32_t> lights;
    for (int i = 0; i < n; ++i)
        if (triangles[i].emissive[0] > 0.0f || triangles[i].emissive[1] > 0.0f || triangles[i].emissive[2] > 0.0f)
            lights.push_back((uint32_t)i);
    if (lights.size() > ((size_t)1 << 26)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "more than 2^26 emissive triangles (the light table is addressed by 32-bit byte offsets)");
    c->n_lights = (int)lights.size();
    c->bvh_height = 0;
    if (n == 0) { c->has_scene = true; return RT_OK; }
    RT_HIP(c, hipMalloc(&c->d_tris, (size_t)n * 60));
    RT_HIP(c, hipMemcpyAsync(c->d_tris, triangles, (size_t)n * 60, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, hipMalloc(&c->d_trimat, (size_t)n * 32));
    k_trimat<<<(n + 255) / 256, 256, 0, c->stream>>>(n, c->d_tris, c->d_trimat);
    RT_HIP(c, hipGetLastError());
    if (c->n_lights > 0)
    {
        uint32_t* d_ids = nullptr;
        RT_HIP(c, hipMalloc(&d_ids, lights.size() * 4));
        RT_HIP(c, hipMemcpyAsync(d_ids, lights.data(), lights.size() * 4, hipMemcpyHostToDevice, c->stream));
        RT_HIP(c, hipMalloc(&c->d_lights, lights.size() * 16 * RT_LIGHT_STRIDE));
        RT_HIP(c, hipMalloc(&c->d_light_ke, lights.size() * 16));
        k_light_table<<<(c->n_lights + 255) / 256, 256, 0, c->stream>>>(c->n_lights, d_ids, c->d_tris, c->d_lights, c->d_light_ke);
        RT_HIP(c, hipGetLastError());
        std::vector<float> w(lights.size());
        for (size_t i = 0; i < lights.size(); ++i) w[i] = light_weight_of(triangles[lights[i]]);
        const int ra = build_light_alias(c, w, d_ids, true, c->stream);
        RT_HIP(c, hipStreamSynchronize(c->stream));
        hipFree(d_ids);
        if (ra != RT_OK) return ra;
    }
    if (c->grid_cells > 0)
    {
        c->h_grid_tris.resize((size_t)n * 15);
        memcpy(c->h_grid_tris.data(), triangles, (size_t)n * 60);
        const int rg = build_light_grid(c, lights, c->stream);
        if (rg != RT_OK) return rg;
    }
    const int rc = build_bvh(c, triangles, n);
    if (rc != RT_OK) return rc;
    { const int rm = kept_vertices_replace(c, keep_vertices); if (rm != RT_OK) return rm; }
    RT_HIP(c, hipStreamSynchronize(c->stream));
    c->build_ms = (float)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_build0).count() * 1e-3f;
    c->h_lights.swap(lights);
    c->has_scene = true;
    return RT_OK;
}

/* Level lists of the wide tree's inner records, top-down from the root (bvh_refit.h); once per scene. */
static int refit_topology(rt_ctx* c)
{
    hipStream_t st = c->stream;
    const int levels = c->wide_height;
    if (levels < 1 || levels > REFIT_MAX_LEVELS) RT_FAIL(c, RT_ERR_STATE, "internal: wide tree height %d", levels);
    const uint32_t cap = (uint32_t)c->n_wide;
    hipFree(c->d_refit_list); hipFree(c->d_refit_box); hipFree(c->d_refit_bounds); /* a failed earlier attempt */
    c->d_refit_list = nullptr; c->d_refit_box = nullptr; c->d_refit_bounds = nullptr;
    RT_HIP(c, hipMalloc(&c->d_refit_list, (size_t)cap * 4));
    RT_HIP(c, hipMalloc(&c->d_refit_box, (size_t)cap * 24));
    RT_HIP(c, hipMalloc(&c->d_refit_bounds, 48)); /* 6 bound keys; from byte 32: the two doubles of k_bvh_cost */
    uint32_t* d_off = nullptr;
    RT_HIP(c, hipMalloc(&d_off, (size_t)(levels + 2) * 4));
    std::vector<uint32_t> off((size_t)levels + 2, 0u);
    off[1] = 1u; /* level 0 = the root, record 0 */
    const uint32_t root = 0u;
    int rc = RT_OK;
    auto ck = [&](hipError_t e) { if (e != hipSuccess && rc == RT_OK) { c->err = std::string("refit topology: ") + hipGetErrorString(e); rc = RT_ERR_HIP; } };
    ck(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    ck(hipMemcpyAsync(c->d_refit_list, &root, 4, hipMemcpyHostToDevice, st));
    /* the scene bounds of the leaves' pad start from the whole scene; updates only grow them */
    ck(hipMemsetAsync(c->d_refit_bounds, 0xff, 12, st));
    ck(hipMemsetAsync(c->d_refit_bounds + 3, 0, 12, st));
    k_refit_bounds<<<(c->n_tris + 255) / 256, 256, 0, st>>>(c->d_tris, c->n_tris, c->d_refit_bounds);
    for (int level = 0; level < levels && rc == RT_OK; ++level)
    {
        /* level l holds at most 4^l records */
        const uint64_t bound = std::min<uint64_t>((uint64_t)1 << std::min(2 * level, 40), cap);
        k_refit_topo_next<<<1, 1, 0, st>>>(level, d_off);
        k_refit_topo<<<(unsigned)((bound + 255) / 256), 256, 0, st>>>(level, d_off, c->d_refit_list, cap, (const uint32_t*)c->d_wide);
        ck(hipGetLastError());
    }
    ck(hipMemcpyAsync(off.data(), d_off, off.size() * 4, hipMemcpyDeviceToHost, st));
    ck(hipStreamSynchronize(st));
    hipFree(d_off);
    if (rc != RT_OK) return rc;
    /* every level non-empty, nothing below the last one, no more inner records than records */
    for (int level = 0; level < levels; ++level)
        if (off[(size_t)level + 1] <= off[(size_t)level]) RT_FAIL(c, RT_ERR_STATE, "internal: wide tree level %d is empty", level);
    if (off[(size_t)levels + 1] != off[(size_t)levels] || off[(size_t)levels] > cap)
        RT_FAIL(c, RT_ERR_STATE, "internal: wide tree deeper than its height %d (or %u inner records of %u)", levels, off[(size_t)levels], cap);
    off.pop_back();
    c->refit_off.swap(off);
    return RT_OK;
}

/* rt_bvh_cost of the tree as it stands: k_bvh_cost over the level lists, its two doubles behind the refit's bounds.
 * bvh_cost_launch enqueues, bvh_cost_read reads them back once the stream has been synchronised. */
static double* bvh_cost_words(rt_ctx* c) { return (double*)(c->d_refit_bounds + 8); }
static int bvh_cost_launch(rt_ctx* c, double h[2])
{
    hipStream_t st = c->stream;
    const uint32_t n_inner = c->refit_off.back();
    RT_HIP(c, hipMemsetAsync(bvh_cost_words(c), 0, 16, st));
    k_bvh_cost<<<(n_inner + 255) / 256, 256, 0, st>>>(c->d_refit_list, n_inner, (const uint32_t*)c->d_wide, bvh_cost_words(c));
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(h, bvh_cost_words(c), 16, hipMemcpyDeviceToHost, st));
    return RT_OK;
}
static double bvh_cost_read(const double h[2]) { return h[1] > 0.0 ? h[0] / h[1] : 0.0; }

int rt_bvh_cost(rt_ctx* c, double* now, double* at_build)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "rt_bvh_cost before rt_scene_set");
    RT_HIP(c, hipSetDevice(c->device));
    double cost = 0.0;
    if (c->d_wide && c->n_wide >= 1) /* else: an empty scene */
    {
        if (c->refit_off.empty()) { const int rc = refit_topology(c); if (rc != RT_OK) return rc; }
        double h[2] = {0.0, 0.0};
        { const int rc = bvh_cost_launch(c, h); if (rc != RT_OK) return rc; }
        RT_HIP(c, hipStreamSynchronize(c->stream));
        cost = bvh_cost_read(h);
    }
    if (now) *now = cost;
    if (at_build) *at_build = c->cost_at_build >= 0.0 ? c->cost_at_build : cost; /* no update yet: the tree is the build's */
    return RT_OK;
}

/* A scene's first update, before the refit writes a record and while d_tris still holds the triangles the build split: the
 * cost of the tree as built, and the fragment table of bvh_refit.h. One host round trip (the cost and the table's size);
 * the table's kernels run ahead of the refit on the stream. The table is an optimisation: if it cannot be made (out of
 * memory, counts that do not match) the update goes on and this scene refits with whole-triangle boxes, which is exact.
 * frag_pending is dropped first: the leaves' words are rewritten at most once. */
static int refit_first_update(rt_ctx* c)
{
    hipStream_t st = c->stream;
    double h[2] = {0.0, 0.0};
    { const int rc = bvh_cost_launch(c, h); if (rc != RT_OK) return rc; }
    const bool want_table = c->frag_pending;
    c->frag_pending = false;
    const int n_tris = c->n_tris;
    const uint32_t n_inner = c->refit_off.back();
    const int gt = (n_tris + 255) / 256;
    const unsigned gi = (n_inner + 255) / 256;
    /* one scratch allocation: fragments per triangle, those of split triangles and their offsets; fragment leaves per inner
     * record and their offsets; the scans' workspace */
    size_t sb0 = 0, sb1 = 0;
    uint32_t* d_tmp = nullptr;
    uint32_t *d_cnt = nullptr, *d_fc = nullptr, *d_foff = nullptr, *d_per = nullptr, *d_sbase = nullptr;
    void* d_scan = nullptr;
    bool table = want_table;
    if (table)
    {
        table = rocprim::exclusive_scan(nullptr, sb0, d_fc, d_foff, 0u, (size_t)n_tris, rocprim::plus<uint32_t>(), st) == hipSuccess &&
                rocprim::exclusive_scan(nullptr, sb1, d_per, d_sbase, 0u, (size_t)n_inner, rocprim::plus<uint32_t>(), st) == hipSuccess;
        const size_t words = 3 * (size_t)n_tris + 2 * (size_t)n_inner + 64;
        table = table && hipMalloc(&d_tmp, words * 4 + std::max(sb0, sb1)) == hipSuccess;
        if (!table) (void)hipGetLastError();
    }
    uint32_t tail[4] = {0, 0, 0, 0};
    if (table)
    {
        d_cnt = d_tmp; d_fc = d_cnt + n_tris; d_foff = d_fc + n_tris; d_per = d_foff + n_tris; d_sbase = d_per + n_inner;
        d_scan = d_tmp + (((3 * (size_t)n_tris + 2 * (size_t)n_inner) + 63) & ~(size_t)63); /* 256-byte aligned */
        /* fragments per split triangle, as the build counted them (same kernel, same triangles, same L) */
        k_split_refs<false><<<gt, 256, 0, st>>>(c->d_tris, n_tris, c->frag_L, c->frag_pad, nullptr, d_cnt, nullptr, nullptr);
        k_frag_counts<<<gt, 256, 0, st>>>(n_tris, d_cnt, d_fc);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = rocprim::exclusive_scan(d_scan, sb0, d_fc, d_foff, 0u, (size_t)n_tris, rocprim::plus<uint32_t>(), st);
        /* fragment leaves per inner record, in the order the refit visits them */
        if (e == hipSuccess) { k_frag_leaves<<<gi, 256, 0, st>>>(c->d_refit_list, n_inner, (const uint32_t*)c->d_wide, d_per); e = hipGetLastError(); }
        if (e == hipSuccess) e = rocprim::exclusive_scan(d_scan, sb1, d_per, d_sbase, 0u, (size_t)n_inner, rocprim::plus<uint32_t>(), st);
        if (e == hipSuccess) e = hipMemcpyAsync(&tail[0], d_foff + n_tris - 1, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&tail[1], d_fc + n_tris - 1, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&tail[2], d_sbase + n_inner - 1, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&tail[3], d_per + n_inner - 1, 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) { hipFree(d_tmp); RT_FAIL(c, RT_ERR_HIP, "fragment table: %s", hipGetErrorString(e)); }
    }
    { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) { hipFree(d_tmp); RT_FAIL(c, RT_ERR_HIP, "first update: %s", hipGetErrorString(e)); } }
    c->cost_at_build = bvh_cost_read(h);
    const uint32_t n_frags = tail[0] + tail[1];
    /* every fragment of a split triangle has its leaf, or the records are not what this build left: no table then */
    table = table && n_frags != 0 && tail[2] + tail[3] == n_frags;
    uint32_t* d_slot_of = nullptr;
    if (table)
    {
        table = hipMalloc(&d_slot_of, (size_t)n_frags * 4) == hipSuccess && hipMalloc(&c->d_frag_uv, (size_t)n_frags * FRAG_MAX_VERTS * 8) == hipSuccess &&
                hipMalloc(&c->d_frag_n, (size_t)n_frags) == hipSuccess;
        if (!table) (void)hipGetLastError();
    }
    if (table)
    {
        hipError_t e = hipMemsetAsync(d_slot_of, 0xff, (size_t)n_frags * 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(c->d_frag_n, 0, (size_t)n_frags, st); /* a slot nobody fills: k_refit_level falls back */
        if (e == hipSuccess)
        {
            k_frag_assign<<<gi, 256, 0, st>>>(c->d_refit_list, n_inner, (uint32_t*)c->d_wide, d_sbase, d_cnt, d_foff, n_frags, n_tris, d_slot_of);
            k_frag_emit<<<gt, 256, 0, st>>>(c->d_tris, n_tris, c->frag_L, d_cnt, d_foff, d_slot_of, n_frags, c->d_frag_uv, c->d_frag_n);
            e = hipGetLastError();
        }
        if (e != hipSuccess) { hipFree(d_tmp); hipFree(d_slot_of); RT_FAIL(c, RT_ERR_HIP, "fragment table: %s", hipGetErrorString(e)); }
        c->n_frags = n_frags;
    }
    else
    {
        hipFree(c->d_frag_uv); hipFree(c->d_frag_n);
        c->d_frag_uv = nullptr; c->d_frag_n = nullptr; c->n_frags = 0;
    }
    hipFree(d_tmp); /* waits for the kernels above */
    hipFree(d_slot_of);
    return RT_OK;
}

/* rt_temporal_light_motion inside rt_scene_update(first, count), after the streams are drained and before anything of the old scene is
 * overwritten (light_follow.h, light_follow_kernels.h). Runs iff the toggle is on and the span holds an emissive
 * triangle in the OLD array; then every physical reservoir buffer whose light samples describe the generation this update ends
 * (HistoryTag::light_current) is re-based in place with its radiance side record, one launch each, and its light_gen advances. With the
 * toggle on and no emissive triangle in the old span nothing is launched and a current buffer stays current (light_untouched). */
static int light_follow_rebase(rt_ctx* c, const rt_triangle* triangles, uint32_t first, uint32_t count)
{
    c->lf_last = 0;
    c->lf_timed = c->light_follow && c->timing;
    c->lf_launched = false;
    if (!c->light_follow) return RT_OK;
    const auto lo = std::lower_bound(c->h_lights.begin(), c->h_lights.end(), first);
    const auto hi = std::lower_bound(lo, c->h_lights.end(), first + count);
    const uint32_t n_ids = (uint32_t)(hi - lo);
    if (n_ids == 0u)
    {
        /* no emitter of the old array changes: the samples of a current buffer stay where they are and stay current */
        for (int p = 0; p < 5; ++p) c->res_tag[p].light_untouched(c->moved.geo_gen);
        return RT_OK;
    }
    int phys[5], np = 0;
    for (int p = 0; p < 5; ++p)
        if (c->d_rec[p] && c->d_rad[p] && c->res_tag[p].light_current(c->moved.geo_gen)) phys[np++] = p;
    if (np == 0) return RT_OK;
    hipStream_t st = c->stream;
    const size_t tri_bytes = (size_t)count * 60, need = tri_bytes + (size_t)n_ids * 4;
    if (need > c->lf_stage_bytes)
    {
        hipFree(c->d_lf_stage);
        c->d_lf_stage = nullptr; c->lf_stage_bytes = 0;
        RT_HIP(c, hipMalloc(&c->d_lf_stage, need));
        c->lf_stage_bytes = need;
    }
    unsigned int* d_box = (unsigned int*)(c->d_lf_words + LF_COUNTER_WORDS);
    RT_HIP(c, hipMemcpyAsync(c->d_lf_stage, triangles, tri_bytes, hipMemcpyHostToDevice, st));
    RT_HIP(c, hipMemcpyAsync((char*)c->d_lf_stage + tri_bytes, &*lo, (size_t)n_ids * 4, hipMemcpyHostToDevice, st));
    RT_HIP(c, hipMemsetAsync(d_box, 0xff, 12, st));
    RT_HIP(c, hipMemsetAsync(d_box + 3, 0, 12, st));
    if (c->lf_timed)
    {
        for (hipEvent_t& e : c->lf_ev) if (!e) RT_HIP(c, hipEventCreate(&e));
        RT_HIP(c, hipEventRecord(c->lf_ev[0], st));
    }
    k_light_follow_box<<<(count + 255) / 256, 256, 0, st>>>(c->d_tris, first, count, d_box);
    LightFollowParams P;
    P.n_records = (uint32_t)local_pixels(c);
    P.first = first; P.count = count;
    P.tris_old = c->d_tris; P.tris_new = (const float*)c->d_lf_stage;
    P.ids = (const uint32_t*)((const char*)c->d_lf_stage + tri_bytes); P.n_ids = n_ids;
    P.wide = c->d_wide; P.n_wide = c->d_wide ? (uint32_t)c->n_wide : 0u;
    P.box = d_box; P.counters = c->d_lf_words;
    const bool direct = (int64_t)n_ids <= (int64_t)c->lf_direct_max;
    const unsigned grid = (P.n_records + BLOCK_THREADS - 1) / BLOCK_THREADS;
    for (int k = 0; k < np && grid > 0u; ++k)
    {
        if (direct) k_light_follow<true><<<grid, BLOCK_THREADS, 0, st>>>(P, c->d_rec[phys[k]], c->d_rad[phys[k]]);
        else k_light_follow<false><<<grid, BLOCK_THREADS, 0, st>>>(P, c->d_rec[phys[k]], c->d_rad[phys[k]]);
        c->res_tag[phys[k]].light_rebased(c->moved.geo_gen);
    }
    RT_HIP(c, hipGetLastError());
    if (c->lf_timed) RT_HIP(c, hipEventRecord(c->lf_ev[1], st));
    c->lf_launched = true;
    c->lf_last = np;
    c->lf_stats0 += (uint64_t)np;
    ++c->res_epoch; /* reservoir buffers written outside the staged frame */
    return RT_OK;
}

int rt_scene_update(rt_ctx* c, const rt_triangle* triangles, uint32_t first, uint32_t count)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "rt_scene_update before rt_scene_set");
    if ((uint64_t)first + count > (uint64_t)c->n_tris)
        RT_FAIL(c, RT_ERR_ARG, "triangles [%u, %llu) outside the scene's %d", first, (unsigned long long)first + count, c->n_tris);
    if (!triangles && count) RT_FAIL(c, RT_ERR_ARG, "null triangles");
    if (count == 0) return RT_OK;
    RT_HIP(c, hipSetDevice(c->device));
    /* every stream that may still read the old scene, as rt_scene_set */
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    if (c->own_stream && c->own_stream != c->stream) RT_HIP(c, hipStreamSynchronize(c->own_stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream));
    drop_look_ahead(c);
    ++c->epoch;
    c->bin_stale = true;
    hipStream_t st = c->stream;
    /* light list: the ids below and above the span stay, the span's are taken from the new triangles (index order) */
    std::vector<uint32_t> lights;
    std::vector<float> light_w; /* the weights likewise: those of the span from the new triangles (rt_light_sampling) */
    bool span_has_light = false;
    {
        const auto lo = std::lower_bound(c->h_lights.begin(), c->h_lights.end(), first);
        const auto hi = std::lower_bound(lo, c->h_lights.end(), first + count); /* <= n_tris: no wrap */
        lights.reserve(c->h_lights.size());
        lights.insert(lights.end(), c->h_lights.begin(), lo);
        light_w.reserve(c->h_lights.size());
        light_w.insert(light_w.end(), c->h_light_w.begin(), c->h_light_w.begin() + (lo - c->h_lights.begin()));
        for (uint32_t i = 0; i < count; ++i)
            if (triangles[i].emissive[0] > 0.0f || triangles[i].emissive[1] > 0.0f || triangles[i].emissive[2] > 0.0f)
            {
                lights.push_back(first + i);
                light_w.push_back(light_weight_of(triangles[i]));
                span_has_light = true;
            }
        lights.insert(lights.end(), hi, c->h_lights.end());
        light_w.insert(light_w.end(), c->h_light_w.begin() + (hi - c->h_lights.begin()), c->h_light_w.end());
    }
    if (lights.size() > ((size_t)1 << 26)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "more than 2^26 emissive triangles (the light table is addressed by 32-bit byte offsets)");
    if (c->refit_off.empty()) { const int rc = refit_topology(c); if (rc != RT_OK) return rc; }
    if (c->cost_at_build < 0.0) { const int rc = refit_first_update(c); if (rc != RT_OK) return rc; }
    /* rt_temporal_light_motion: the old triangles and the old tree are still in place here */
    { const int rc = light_follow_rebase(c, triangles, first, count); if (rc != RT_OK) return rc; }
    /* rt_temporal_motion / rt_denoise_temporal_motion: d_tv still holds the old vertices here. A history (a reservoir buffer for the
     * first, the denoiser's for the second) written since the last update by a consumer whose toggle is on carries the
     * generation this update ends: d_tv_prev is brought to it (it differs from d_tv over the old moved range only) and a new range
     * starts. Otherwise no history of the generations in between exists, and the range grows to cover this span too. */
    const MovedUpdate mu = c->moved.update(first, count);
    if (mu.kind == MovedUpdate::REBASE && mu.hi > mu.lo)
        RT_HIP(c, hipMemcpyAsync(c->d_tv_prev + 3 * (size_t)mu.lo, c->d_tv + 3 * (size_t)mu.lo, (size_t)(mu.hi - mu.lo) * 48, hipMemcpyDeviceToDevice, st));
    /* per-triangle arrays of the span */
    RT_HIP(c, hipMemcpyAsync(c->d_tris + 15 * (size_t)first, triangles, (size_t)count * 60, hipMemcpyHostToDevice, st));
    const int gs = (int)((count + 255) / 256);
    k_trimat<<<gs, 256, 0, st>>>((int)count, c->d_tris + 15 * (size_t)first, c->d_trimat + 2 * (size_t)first);
    k_bvh_tv<<<gs, 256, 0, st>>>(c->d_tris + 15 * (size_t)first, (int)count, c->d_tv + 3 * (size_t)first);
    RT_HIP(c, hipGetLastError());
    /* light table: records hold positions and 1 / n_lights, so all of it is rebuilt (k_light_table, as rt_scene_set) */
    if (lights.size() != c->h_lights.size())
    {
        hipFree(c->d_lights); hipFree(c->d_light_ke); hipFree(c->d_light_ids);
        c->d_lights = nullptr; c->d_light_ke = nullptr; c->d_light_ids = nullptr;
        if (!lights.empty())
        {
            RT_HIP(c, hipMalloc(&c->d_lights, lights.size() * 16 * RT_LIGHT_STRIDE));
            RT_HIP(c, hipMalloc(&c->d_light_ke, lights.size() * 16));
        }
    }
    if (!lights.empty())
    {
        bool upload = lights != c->h_lights;
        if (!c->d_light_ids) { RT_HIP(c, hipMalloc(&c->d_light_ids, lights.size() * 4)); upload = true; }
        if (upload) RT_HIP(c, hipMemcpyAsync(c->d_light_ids, lights.data(), lights.size() * 4, hipMemcpyHostToDevice, st));
        k_light_table<<<((int)lights.size() + 255) / 256, 256, 0, st>>>((int)lights.size(), c->d_light_ids, c->d_tris, c->d_lights, c->d_light_ke);
        RT_HIP(c, hipGetLastError());
    }
    /* the alias table: only if a weight or the list can have changed (the span holds a light now, or held one) */
    if (span_has_light || lights != c->h_lights)
    {
        const int ra = build_light_alias(c, light_w, c->d_light_ids, lights.size() != c->h_lights.size(), st);
        if (ra != RT_OK) return ra;
    }
    /* rt_light_grid: the span goes into the host copy; the tables are rebuilt if the span holds or held a light (weights, vertices or
     * the list can have changed) or the scene's bounds moved, and stay otherwise */
    if (c->grid_cells > 0)
    {
        memcpy(c->h_grid_tris.data() + 15 * (size_t)first, triangles, (size_t)count * 60);
        bool rebuild = span_has_light || lights != c->h_lights || !c->grid_built;
        if (!rebuild)
        {
            LightGrid b;
            grid_build_bounds(b, c->h_grid_tris.data(), 15, (size_t)c->n_tris, c->grid_cells);
            rebuild = memcmp(b.lo, c->h_grid.lo, 12) != 0 || memcmp(b.hi, c->h_grid.hi, 12) != 0;
        }
        if (rebuild)
        {
            const int rg = build_light_grid(c, lights, st);
            if (rg != RT_OK) return rg;
        }
    }
    c->n_lights = (int)lights.size();
    /* refit: the pad's bounds grown by the span, then the inner records level by level, deepest first */
    k_refit_bounds<<<gs, 256, 0, st>>>(c->d_tris + 15 * (size_t)first, (int)count, c->d_refit_bounds);
    for (int level = (int)c->refit_off.size() - 2; level >= 0; --level)
    {
        const uint32_t b = c->refit_off[(size_t)level], m = c->refit_off[(size_t)level + 1] - b;
        k_refit_level<<<(m + 255) / 256, 256, 0, st>>>(c->d_refit_list + b, m, c->d_tris, c->d_refit_bounds, c->d_refit_box, (uint32_t*)c->d_wide,
                                                        c->n_frags ? c->d_frag_uv : nullptr, c->d_frag_n, c->n_frags);
    }
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipStreamSynchronize(st)); /* the caller's triangles and the light list are host memory */
    c->h_lights.swap(lights);
    return RT_OK;
}

int rt_scene_info(rt_ctx* c, uint32_t* n_triangles, uint32_t* n_lights, uint32_t* bvh_height)
{
    RT_CHECK_CTX(c);
    if (n_triangles) *n_triangles = (uint32_t)c->n_tris;
    if (n_lights) *n_lights = (uint32_t)c->n_lights;
    if (bvh_height) *bvh_height = (uint32_t)c->bvh_height;
    return RT_OK;
}
int rt_build_ms(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    *ms = c->build_ms;
    return RT_OK;
}
int rt_bvh_info(rt_ctx* c, uint32_t* n_refs, uint32_t* n_nodes, uint32_t* wide_height)
{
    RT_CHECK_CTX(c);
    if (wide_height) *wide_height = (uint32_t)c->wide_height;
    if (n_refs) *n_refs = (uint32_t)c->n_refs;
    if (n_nodes) *n_nodes = (uint32_t)c->n_wide;
    return RT_OK;
}

/* common/camera.hpp:11-25 (host; tan of a float argument = tanf) */
int rt_camera_lookat(rt_ctx* c, const float eye[3], const float center[3], const float up[3], float fovy)
{
    RT_CHECK_CTX(c);
    if (!eye || !center || !up) RT_FAIL(c, RT_ERR_ARG, "null camera vector");
    rt_host::raygen_lookat(&c->rg, eye, center, up, fovy, c->W, c->H); /* host_path.h: shared with the host-only config #1 */
    memcpy(c->eye, eye, 12);
    memcpy(c->cam_eye, eye, 12);
    memcpy(c->cam_at, center, 12);
    c->cam_fovy = fovy;
    c->has_camera = true;
    ++c->epoch;
    return RT_OK;
}
/* ---- interactive camera of the examples (common/misc.hpp:108-224 CameraControl): the mouse
 * callbacks restated as explicit calls; the window system stays out of scope. Each call updates
 * eye / look-at, re-derives the RayGenerator (fovy and up as last set) and raises the `updated`
 * flag that the frame loop turns into a `clear` (10_restir_di.cpp:257-267). ---- */
static void camera_refresh(rt_ctx* c)
{
    const float up[3] = {0.0f, 1.0f, 0.0f};
    rt_camera_lookat(c, c->cam_eye, c->cam_at, up, c->cam_fovy);
    c->cam_updated = true;
}
/* left-button drag by (dx, dy) pixels: orbit around the look-at point (misc.hpp:147-181) */
int rt_camera_orbit(rt_ctx* c, float dx, float dy)
{
    RT_CHECK_CTX(c);
    if (!c->has_camera) RT_FAIL(c, RT_ERR_STATE, "set the camera first");
    float lx = c->cam_eye[0] - c->cam_at[0], ly = c->cam_eye[1] - c->cam_at[1], lz = c->cam_eye[2] - c->cam_at[2];
    const float r = sqrtf(lx * lx + ly * ly + lz * lz);
    const float sensitivity = 0.004f;
    {
        const float st = sinf(dx * sensitivity), ct = cosf(dx * sensitivity);
        const float nx = ct * lx - st * lz, nz = st * lx + ct * lz;
        lx = nx; lz = nz;
    }
    {
        const float xz = sqrtf(lx * lx + lz * lz);
        const float st = sinf(dy * sensitivity), ct = cosf(dy * sensitivity);
        const float new_xz = ct * xz - st * ly, new_y = st * xz + ct * ly;
        if (-r + r * 0.01f < new_y && new_y < r - r * 0.01f)
        {
            lx = lx * (new_xz / xz); lz = lz * (new_xz / xz); ly = new_y;
        }
    }
    c->cam_eye[0] = c->cam_at[0] + lx; c->cam_eye[1] = c->cam_at[1] + ly; c->cam_eye[2] = c->cam_at[2] + lz;
    camera_refresh(c);
    return RT_OK;
}
/* right-button drag: dolly towards / away from the look-at point (misc.hpp:183-190) */
int rt_camera_zoom(rt_ctx* c, float dy)
{
    RT_CHECK_CTX(c);
    if (!c->has_camera) RT_FAIL(c, RT_ERR_STATE, "set the camera first");
    const float lx = c->cam_eye[0] - c->cam_at[0], ly = c->cam_eye[1] - c->cam_at[1], lz = c->cam_eye[2] - c->cam_at[2];
    const float r = sqrtf(lx * lx + ly * ly + lz * lz);
    const float sensitivity = 0.002f;
    const float new_r = fmaxf(r - r * sensitivity * dy, 0.01f);
    const float s = new_r / r;
    c->cam_eye[0] = c->cam_at[0] + lx * s; c->cam_eye[1] = c->cam_at[1] + ly * s; c->cam_eye[2] = c->cam_at[2] + lz * s;
    camera_refresh(c);
    return RT_OK;
}
/* middle-button drag: pan eye and look-at in the view plane (misc.hpp:192-205) */
int rt_camera_pan(rt_ctx* c, float dx, float dy)
{
    RT_CHECK_CTX(c);
    if (!c->has_camera) RT_FAIL(c, RT_ERR_STATE, "set the camera first");
    const f3 eye = F3(c->cam_eye[0], c->cam_eye[1], c->cam_eye[2]), at = F3(c->cam_at[0], c->cam_at[1], c->cam_at[2]);
    const float r = length(eye - at);
    const float sensitivity = 0.001f;
    const f3 forward = normalize(at - eye);
    const f3 right = normalize(cross(forward, F3(0.0f, 1.0f, 0.0f)));
    const f3 up = cross(right, forward);
    const float amount = fmaxf(r * sensitivity, 0.01f);
    const f3 delta = (-right) * dx * amount + up * dy * amount;
    const f3 e2 = eye + delta, a2 = at + delta;
    c->cam_eye[0] = e2.x; c->cam_eye[1] = e2.y; c->cam_eye[2] = e2.z;
    c->cam_at[0] = a2.x; c->cam_at[1] = a2.y; c->cam_at[2] = a2.z;
    camera_refresh(c);
    return RT_OK;
}
/* CameraControl::is_updated(): returns the flag and clears it */
int rt_camera_updated(rt_ctx* c, int* updated)
{
    RT_CHECK_CTX(c);
    if (!updated) return RT_ERR_ARG;
    *updated = c->cam_updated ? 1 : 0;
    c->cam_updated = false;
    return RT_OK;
}
int rt_camera_pose(rt_ctx* c, float eye[3], float lookat[3])
{
    RT_CHECK_CTX(c);
    if (eye) memcpy(eye, c->cam_eye, 12);
    if (lookat) memcpy(lookat, c->cam_at, 12);
    return RT_OK;
}

int rt_camera_set(rt_ctx* c, const rt_raygen* rg, const float eye[3])
{
    RT_CHECK_CTX(c);
    if (!rg || !eye) RT_FAIL(c, RT_ERR_ARG, "null raygen/eye");
    c->rg = *rg;
    c->eye[0] = eye[0]; c->eye[1] = eye[1]; c->eye[2] = eye[2];
    c->has_camera = true;
    ++c->epoch;
    return RT_OK;
}
int rt_camera_get(rt_ctx* c, rt_raygen* rg)
{
    RT_CHECK_CTX(c);
    if (!rg) return RT_ERR_ARG;
    *rg = c->rg;
    return RT_OK;
}
int rt_options_set(rt_ctx* c, const rt_options* o)
{
    RT_CHECK_CTX(c);
    if (!o) RT_FAIL(c, RT_ERR_ARG, "null options");
    if (o->ris_sample_count < 0 || o->spatial_resampling_sample_count < 0 || o->spatial_resampling_passes < 0)
        RT_FAIL(c, RT_ERR_ARG, "negative counts in options");
    {
        /* The 64-B record keeps M in 30 bits (rt_device.h; the reference's int M has 31). The largest M a
         * frame can reach is 21 * ris (candidates + the temporal cap of 20 * ris, 10_restir_di.cu:185-187)
         * times (1 + neighbours) per spatial pass: refuse option sets that could wrap instead of wrapping. */
        double m = 21.0 * (double)(o->ris_sample_count > 0 ? o->ris_sample_count : 1);
        for (int k = 0; k < o->spatial_resampling_passes && m < 4e9; ++k) m *= 1.0 + (double)o->spatial_resampling_sample_count;
        if (m >= 1073741824.0)
            RT_FAIL(c, RT_ERR_UNSUPPORTED, "options let the reservoir count M reach %.3g >= 2^30 (ris_sample_count %d, %d neighbours, %d passes)",
                    m, o->ris_sample_count, o->spatial_resampling_sample_count, o->spatial_resampling_passes);
    }
    c->opt = *o;
    ++c->epoch;
    return RT_OK;
}
int rt_options_get(rt_ctx* c, rt_options* o)
{
    RT_CHECK_CTX(c);
    if (!o) return RT_ERR_ARG;
    *o = c->opt;
    return RT_OK;
}

#define NEED_SCENE(c)                                                               \
    if (!(c)->has_scene || !(c)->has_camera) RT_FAIL(c, RT_ERR_STATE, "scene and camera must be set first");
#define NEED_RES(c, id) \
    if ((id) < 0 || (id) > 2) RT_FAIL(c, RT_ERR_ARG, "bad reservoir buffer id %d", (id));

static int launch_grid(const rt_ctx* c, const Launch& L) { return tile_grid(c->W, L.row1 - L.row0, TILE_W, TILE_H, L.rowb1 - L.rowb0); }
/* The work-sharing walk evens out the per-wavefront tail (longest lane 8x the mean: profiles/r02_wave_tail.txt). A launch
 * of many rounds of wavefronts hides that tail behind the next wavefronts and only pays the bookkeeping; a launch of
 * about one round (a strip of the multi-GPU frame: 135 rows x 1920 = 4050 wavefronts on 1024 SIMDs x 4-5) ends with
 * its slowest wavefront and runs ~2x faster with it. */
#ifndef RT_WS_AUTO_WAVES
#define RT_WS_AUTO_WAVES 12288
#endif
static bool use_ws(const rt_ctx* c, int grid) { return c->tune_ws < 0 ? grid <= RT_WS_AUTO_WAVES : c->tune_ws != 0; }
#ifndef RT_WS_PRIMARY_AUTO_WAVES
#define RT_WS_PRIMARY_AUTO_WAVES 8192
#endif
static bool use_ws_primary(const rt_ctx* c, int grid) { return c->tune_ws_primary < 0 ? grid <= RT_WS_PRIMARY_AUTO_WAVES : c->tune_ws_primary != 0; }
/* grid of the tracing kernels: TRACE_BLOCK threads on TileShape<TRACE_BLOCK> tiles */
/* priority of a side stream: 0 = default, +1 = lowest, -1 = highest (the range HIP reports), overridable for A/B runs */
static int stream_priority(const char* env, int dflt)
{
    const char* e = getenv(env);
    int want = e ? atoi(e) : dflt;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
    return want > 0 ? least : (want < 0 ? greatest : 0);
}
static bool use_tail(const rt_ctx* c, bool timed)
{
    if (timed) return false; /* rt_timing brackets the kernels with events on the main stream */
    /* auto = always (r03: strips 0.442 -> 0.373 ms per frame at 1080p in 8 strips; a whole 1080p frame 1.68 -> 1.63 ms) */
    return c->tune_tail != 0;
}
/* the stream about to be used waits for the previous frame's resolve + tone_mapping (no-op unless they are in flight) */
static int join_tail(rt_ctx* c, const Launch& L)
{
    if (!c->tail.pending_main) return RT_OK;
    RT_HIP(c, hipStreamWaitEvent(L.stream, c->tail.ev, 0));
    /* the second lane of a stage waits for itself; the main stream still has to */
    if (L.stream != c->aux_stream) c->tail.pending_main = false;
    return RT_OK;
}
/* the entry points outside the staged frame: the context's current stream joins */
#define JOIN_TAIL(c) do { const int _jt = join_tail(c, whole_launch(c)); if (_jt != RT_OK) return _jt; } while (0)
/* a kernel of the staged frame that WRITES reservoir buffer `phys` (and reads only what the tail reads too): it waits for the
 * tail only if that is the buffer the tail reads */
static int join_tail_for(rt_ctx* c, const Launch& L, int phys) { return (c->tail.pending_main && phys == c->tail.phys) ? join_tail(c, L) : RT_OK; }
/* the pipelined stage 0 (ahead.stream) may still be running when a call outside the staged frame — or a frame that does not
 * take its results — starts to write what it reads (the history buffer, the other G-buffer set) or reads what it writes: the
 * stream about to be used waits for it first (cheap: that work is behind already). ADVICE r03. */
static int join_spec(rt_ctx* c, const Launch& L)
{
    if (!c->ahead.outstanding) return RT_OK;
    RT_HIP(c, hipStreamWaitEvent(L.stream, c->ahead.ev_done, 0));
    if (L.stream != c->aux_stream) c->ahead.outstanding = false;
    return RT_OK;
}
#define JOIN_SPEC(c) do { const int _js = join_spec(c, whole_launch(c)); if (_js != RT_OK) return _js; } while (0)
static int trace_grid(const rt_ctx* c, const Launch& L)
{
    return tile_grid(c->W, L.row1 - L.row0, TileShape<TRACE_BLOCK>::W, TileShape<TRACE_BLOCK>::H, L.rowb1 - L.rowb0);
}

/* rt_clear over the launch's rows */
static int clear_rows(rt_ctx* c, const Launch& L)
{
    { const int rc = join_tail(c, L); if (rc != RT_OK) return rc; }
    k_clear<<<launch_grid(c, L), BLOCK, 0, L.stream>>>(make_params(c, L, 0, 0), c->d_accum);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_clear(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    return clear_rows(c, whole_launch(c));
}

/* the raycast launch of the context's tuning, into the launch's G-buffer set */
static void launch_raycast(rt_ctx* c, const Launch& L)
{
    const int g = trace_grid(c, L);
    const FrameParams P = make_params(c, L, 0, 0, K_RAYCAST);
#ifdef RT_EXPERIMENTS
    if (c->tune_half_raycast) { k_raycast_half<<<2 * g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), P, L.vis, L.g0, L.g1); return; }
    if (c->tune_ws_primary == 2) { k_raycast_quad<<<4 * g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), P, L.vis, L.g0, L.g1); return; }
#endif
    if (use_ws_primary(c, g)) k_raycast<true><<<g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), P, L.vis, L.g0, L.g1);
    else k_raycast<false><<<g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), P, L.vis, L.g0, L.g1);
}
/* The current G-buffer set has new content: its serial and its shaded bits are new, however it got there */
enum { GBUF_TRACED = 0, GBUF_TAKEN = 1, GBUF_UPLOADED = 2 };
static void gbuffer_written(rt_ctx* c, const Launch& L, int how)
{
    c->gbuf.valid = c->gbuf.shaded_bits_stale = true;
    ++c->gbuf.serial;
    if (how == GBUF_UPLOADED) return; /* k_gbuffer_from_vis is not a trace: the caller bumps `epoch`, and no epoch here follows it */
    c->gbuf.epoch = c->epoch;
    /* taken: the look-ahead traced it under ahead.epoch == epoch (look_ahead_usable), all owned rows, on ahead.stream, and counted it when it was launched */
    if (how == GBUF_TAKEN) { c->gbuf.traced_epoch = c->epoch; c->gbuf.ahead_ordered = true; return; }
    /* a launch on L.stream has traced primary rays into the CURRENT G-buffer set (rt_primary_launches counts it): over all owned rows it
     * makes the set the answer for `epoch` (gbuffer_reusable); over a sub-range it leaves gbuf.traced_epoch alone — either the set was
     * the answer already and the rows got the same bytes, or it is of an older epoch, which never comes back */
    ++c->gbuf.primary_launches;
    if (covers_owned_rows(c, L)) c->gbuf.traced_epoch = c->epoch;
    if (L.stream != c->ahead.stream) c->gbuf.ahead_ordered = false;
}
/* r13 (rt_gbuffer_reuse): stage 0 of a staged frame needs no primary rays — the current set holds what they would write. Whole-frame
 * contexts only (a strip's marks wait for the raycast's event, and r05 bounded the gain there at 0-9 % of a strip's frame); not while
 * rt_walk_stats counts (the counters of slot 0 are the raycast's). */
static bool gbuffer_reusable(const rt_ctx* c)
{
    return c->gbuf.reuse && whole_frame(c) && !c->walk_on && c->gbuf.valid && c->gbuf.traced_epoch == c->epoch;
}
/* rt_raycast over the launch's rows, with everything it does to the context's state */
static int raycast_rows(rt_ctx* c, const Launch& L)
{
    int rc = join_tail(c, L);
    if (rc == RT_OK) rc = join_spec(c, L);
    if (rc != RT_OK) return rc;
    NEED_SCENE(c);
    launch_raycast(c, L);
    RT_HIP(c, hipGetLastError());
    gbuffer_written(c, L, GBUF_TRACED);
    /* halo rows of the G-buffer keep the neighbours' shaded flags: they stay valid until the camera,
     * the scene or the options change (halo_flags_epoch), which is when the neighbours' G-buffers change */
    return RT_OK;
}
int rt_raycast(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    return raycast_rows(c, whole_launch(c));
}

/* A/B r02 (profiles/r02_next_raycast_ab.txt): a strip's frame is a chain of small launches and exchanges with idle
 * slots the raycast fills (-6 % at 1080p in 8 strips, -3 % at 4K); a whole frame gains < 1 % at 1080p (the overlapped
 * spatial pass just waits for the machine) and its per-kernel times stop being comparable, so auto means strips only */
static bool use_next_raycast(const rt_ctx* c, bool timed)
{
    if (c->tune_spec >= 0) return c->tune_spec != 0;
    /* auto: strips always; whole frames too (r03: with the candidates pipelined as well a 1080p frame gains 3 %), except
     * while rt_timing brackets the kernels of a frame with events — then they run back to back on one stream */
    return !whole_frame(c) || !timed;
}
/* the next frame's generate_candidate(+temporal) too. Not while per-kernel timing is on (rt_timing attributes events of the
 * main stream to kernels) and not with the deferred-visibility queue (its counters live per lane of the main frame). */
static bool use_next_generate(const rt_ctx* c, bool timed)
{
    if (!use_next_raycast(c, timed) || timed || c->tune_defer_vis) return false;
    return c->tune_spec < 0 || c->tune_spec == 2;
}
/* r05, rt_tuning key 22. auto: strips — their kernels are launches of one to three generations of wavefronts and what fills the GPU
 * is running several of them side by side (rank 4 of 8: 1080p 0.306 -> 0.287 ms, 4K 0.889 -> 0.870, profiles/r05_spec_free_ab.txt);
 * a whole frame's kernels fill the GPU alone and only take slots from each other (pipelined 1080p frame 1.277 -> 1.296 ms) */
static bool spec_free(const rt_ctx* c) { return c->tune_spec_free < 0 ? !whole_frame(c) : c->tune_spec_free != 0; }
static int launch_generate(rt_ctx* c, const Launch& L, int frame, int dst_phys, int prev_phys, bool fuse, float4* raycast_vis = nullptr, bool staged = false);
/* r05, rt_tuning key 25: raycast + generate_candidate (+ temporal merge) of a frame in ONE launch — the candidates need the primary ray
 * of their own pixel only, and two launches on a stream cost the first one's ramp-down (its last wavefront starts at 216 of 257 us).
 * The product's fused candidate kernel only (temporal merge on, unshadowed, work-sharing shadow walk), whole owned rows.
 * auto = whole-frame contexts (a strip's marks wait for the G-buffer alone). */
static bool use_fused_stage0(const rt_ctx* c)
{
    const int want = c->tune_fuse_raycast < 0 ? (whole_frame(c) ? 1 : 0) : c->tune_fuse_raycast;
    /* r06: also while rt_timing brackets the kernels — the events then bracket the ONE launch the headline frames run
     * (ms[1] = the empty bracket where the raycast launch would be, ms[2] = the launch; rt_stage0_one_launch says which
     * form the timed frame ran). rt_tuning 25 = 0 times the two kernels. */
    if (!want) return false;
#ifdef RT_EXPERIMENTS
    if (c->tune_half_raycast || c->tune_defer_vis || c->tune_ris_pipe) return false;
#endif
    const int g = trace_grid(c, whole_launch(c));
    return c->opt.use_temporal_resampling && !c->opt.use_shadowed_target_function && c->n_lights > 0 && use_ws(c, g) && !use_ws_primary(c, g);
}
/* the next frame's primary rays, behind everything enqueued on the main stream so far, on the stream of their own */
static int launch_next_raycast(rt_ctx* c, int frame)
{
    c->ahead.gen_valid = false;
    if (!use_next_raycast(c, c->timing)) { drop_look_ahead(c); return RT_OK; }
    const bool next_generate = use_next_generate(c, c->timing);
    /* r13: the set the running frame reads is the next frame's too (gbuffer_reusable): the look-ahead is the candidates alone, reading
     * set cur; set o is neither written nor, in a steady run, ever allocated, and the take does not rotate cur */
    const bool reuse = gbuffer_reusable(c);
    if (reuse && !(next_generate && c->n_lights > 0)) { drop_look_ahead(c); return RT_OK; } /* nothing to run ahead */
    const size_t n = local_pixels(c);
    const int o = reuse ? c->gbuf.cur : (c->gbuf.cur + 1) % rt_ctx::NGSET;
    bool fresh_set = false;
    if (!c->gbuf.set[o][0])
    {
        for (int k = 0; k < 3; ++k) RT_HIP(c, hipMalloc(&c->gbuf.set[o][k], n * 16));
        /* halo rows of g1 hold the neighbours' shaded flags (rt_halo_flags_unpack keeps every set current from here on) */
        for (int k = 0; k < 3; ++k) RT_HIP(c, hipMemcpyAsync(c->gbuf.set[o][k], c->gbuf.set[c->gbuf.cur][k], n * 16, hipMemcpyDeviceToDevice, c->stream));
        fresh_set = true;
    }
    /* What this stage 0 needs from the main stream. If the current frame's stage 0 ran there (a cold frame, the first frames,
     * per-kernel timing), its candidates are the history read below: behind everything enqueued on the main stream so far. If the
     * current frame TOOK its stage 0 from this very stream (steady state), nothing: the history was written here, and the set /
     * buffer overwritten below were last read two resolves ago (r05) — the look-ahead runs on, beside whatever the main and the
     * tail stream are doing. (r04 waited here for the main stream, i.e. for the previous frame's passes, and for the previous
     * frame's resolve: raycast(f+2) could not start before resolve(f) had ended.) */
    /* r13: candidates that read the current set wait for the main stream also where a launch there wrote that set last */
    if (!c->frame.gen_taken || fresh_set || !spec_free(c) || (reuse && !c->gbuf.ahead_ordered))
    {
        RT_HIP(c, hipEventRecord(c->ahead.ev_go, c->stream));
        RT_HIP(c, hipStreamWaitEvent(c->ahead.stream, c->ahead.ev_go, 0));
        c->gbuf.ahead_ordered = true; /* whatever wrote set cur was enqueued before this point */
    }
    /* the G-buffer set and the spare reservoir buffer written below: last read by the resolve before the latest one (the set of
     * frame f-2; the buffer that left the roles when frame f-1 was taken) — or earlier */
    /* With ONE resolve on record the free-running form waits for it too (that it need not rested on the main-stream
     * wait above being forced at that point — one frame of overlap, once, buys an invariant that does not depend on it). */
    if (c->tail.n_resolved >= 1)
        RT_HIP(c, hipStreamWaitEvent(c->ahead.stream, c->tail.ev_resolved[(spec_free(c) && c->tail.n_resolved >= 2) ? 1 : 0], 0));
    /* the invariants the free-running look-ahead rests on, checked where it writes (cheap integer tests, every build): the set it
     * overwrites is not the one the running frame reads, and the candidates' buffer has no role in the running frame nor is it
     * what the tail in flight reads */
    if (!reuse && o == c->gbuf.cur) RT_FAIL(c, RT_ERR_STATE, "look-ahead stage 0 would overwrite the running frame's G-buffer set %d", o);
    /* r04's dependencies (not spec_free) hand the tail's buffer over and wait for the latest resolve above */
    if (next_generate && !roles_spare_free(c->frame, (spec_free(c) && c->tail.pending_main) ? c->tail.phys : -1))
        RT_FAIL(c, RT_ERR_STATE, "look-ahead candidates' buffer %d is in use (X %d Y %d Z %d quarantine %d tail %d)", c->frame.spare, c->frame.X, c->frame.Y, c->frame.Z, c->frame.quarantine, c->tail.pending_main ? c->tail.phys : -1);
    Launch spec = whole_launch(c); /* all owned rows, on the stream of its own, into set o */
    spec.stream = c->ahead.stream; spec.vis = c->gbuf.set[o][0]; spec.g0 = c->gbuf.set[o][1]; spec.g1 = c->gbuf.set[o][2];
    const bool one_launch = !reuse && next_generate && use_fused_stage0(c); /* the candidates' launch below traces the primary rays too */
    if (!reuse)
    {
        if (c->timing) hipEventRecord(c->ahead.ev_t[o][0], spec.stream);
        if (!one_launch) launch_raycast(c, spec);
        RT_HIP(c, hipGetLastError());
        if (c->timing) hipEventRecord(c->ahead.ev_t[o][1], spec.stream);
        c->ahead.timed[o] = c->timing;
        ++c->gbuf.primary_launches; /* into set o: it becomes the current set, and gbuf.traced_epoch its epoch, at the take */
    }
    if (next_generate && c->n_lights > 0)
    {
        /* candidates (+ temporal merge) of frame + 1: G-buffer = the set just traced, history = the buffer this frame's
         * stage 0 wrote (c->frame.Y), output = the spare buffer; all owned rows, on the same stream behind the raycast */
        if (!c->d_rec[c->frame.spare])
        {
            RT_HIP(c, hipMalloc(&c->d_rec[c->frame.spare], n * 64));
            RT_HIP(c, hipMalloc(&c->d_rad[c->frame.spare], n * 16));
            RT_HIP(c, hipMemsetAsync(c->d_rec[c->frame.spare], 0, n * 64, spec.stream));
            RT_HIP(c, hipMemsetAsync(c->d_rad[c->frame.spare], 0, n * 16, spec.stream));
        }
        c->ahead.gen_tag = next_ownv_tag(c); /* the frame that takes these candidates continues under their tag */
        spec.tag = c->ahead.gen_tag;
        const int rc = launch_generate(c, spec, frame + 1, c->frame.spare, c->frame.Y, c->opt.use_temporal_resampling != 0, one_launch ? spec.vis : nullptr, true);
        if (rc != RT_OK) return rc;
        c->ahead.gen_valid = true;
        c->ahead.gen_frame = frame + 1;
        c->ahead.gen_hist = c->frame.Y;
        c->ahead.res_epoch = c->res_epoch;
    }
    RT_HIP(c, hipEventRecord(c->ahead.ev_done, spec.stream));
    c->ahead.outstanding = true;
    c->ahead.valid = true;
    c->ahead.reuse = reuse;
    c->ahead.epoch = c->epoch;
    return RT_OK;
}
/* what stage 0 learned: deferred = its primary rays are traced by the candidates' launch; reused (r13) = by nobody, the current G-buffer
 * set is still the answer (gbuffer_reusable); taken = its candidates came from the look-ahead (frame.gen_taken keeps that for the later stages) */
struct Stage0 { bool deferred = false, reused = false, taken = false; };
/* is the look-ahead still the right one for this launch? One that read the current set (ahead.reuse) is good for as long as that set is */
static bool look_ahead_usable(const rt_ctx* c, const Launch& L) { return covers_owned_rows(c, L) && use_next_raycast(c, L.timed) && c->ahead.valid && c->ahead.epoch == c->epoch && (!c->ahead.reuse || gbuffer_reusable(c)); }
/* ... and its candidates: made for this frame, from the buffer that is this frame's history, and no reservoir buffer written outside since */
static bool look_ahead_candidates_usable(const rt_ctx* c, const Launch& L, int frame) { return c->ahead.gen_valid && use_next_generate(c, L.timed) && c->ahead.gen_frame == frame && c->ahead.res_epoch == c->res_epoch && c->ahead.gen_hist == c->frame.X; }
/* the set the look-ahead traced becomes the current one, the context's and the launch's */
static void rotate_gbuffer_set(rt_ctx* c, Launch& L)
{
    c->gbuf.cur = (c->gbuf.cur + 1) % rt_ctx::NGSET;
    L.vis = c->gbuf.vis = c->gbuf.set[c->gbuf.cur][0]; L.g0 = c->gbuf.g0 = c->gbuf.set[c->gbuf.cur][1]; L.g1 = c->gbuf.g1 = c->gbuf.set[c->gbuf.cur][2];
}
/* stage 0's raycast over all owned rows: the G-buffer traced beside the previous frame if it is still the right one */
/* L: the stage's launch; a take moves it to the taken G-buffer set and, with the candidates, to their tag */
static int raycast_or_take(rt_ctx* c, Launch& L, int frame, bool may_defer, Stage0& got)
{
    c->ahead.timed_set = -1;
    c->frame.gen_taken = false;
    if (look_ahead_usable(c, L))
    {
        const bool traced = !c->ahead.reuse; /* the look-ahead traced set cur + 1; otherwise only its candidates are taken */
        if (traced) rotate_gbuffer_set(c, L);
        else got.reused = true;
        RT_HIP(c, hipStreamWaitEvent(L.stream, c->ahead.ev_done, 0));
        c->ahead.outstanding = false;
        if (look_ahead_candidates_usable(c, L, frame))
        {
            roles_take(c->frame, c->opt.spatial_resampling_passes, spec_free(c));
            c->frame.gen_taken = got.taken = true;
            c->frame.tag = c->ahead.gen_tag; /* own-visibility flags of the candidates were written under this tag */
            L.tag = c->frame.tag;
        }
        drop_look_ahead(c);
        if (!traced) return RT_OK; /* the same set, its serial and its shaded bits; the candidates carry its serial (launch_generate) */
        gbuffer_written(c, L, GBUF_TAKEN);
        if (got.taken) c->res_tag[c->frame.Y].gserial = c->gbuf.serial; /* the candidates were made from this G-buffer set */
        if (c->ahead.timed[c->gbuf.cur]) c->ahead.timed_set = c->gbuf.cur;
        return RT_OK;
    }
    drop_look_ahead(c);
    if (gbuffer_reusable(c))
    {
        /* nothing is written: the tail may go on reading the set; a look-ahead that was not taken may still be running on the
         * history and the spare buffer */
        const int rc = join_spec(c, L);
        got.reused = rc == RT_OK;
        return rc;
    }
    if (may_defer)
    {
        /* rt_raycast without its launch: the candidates' kernel of this stage traces the primary rays (use_fused_stage0) */
        int rc = join_tail(c, L);
        if (rc == RT_OK) rc = join_spec(c, L);
        if (rc != RT_OK) return rc;
        gbuffer_written(c, L, GBUF_TRACED); /* the candidates' launch of this stage, all owned rows (may_defer) */
        got.deferred = true;
        return RT_OK;
    }
    return raycast_rows(c, L);
}

/* the hint buffer of the staged frame's candidates (rt_occluder_hints), made on first use; nullptr = switched off */
static int staged_hints(rt_ctx* c, int** hints)
{
    *hints = nullptr;
    if (!c->hints_on || !c->d_tv) return RT_OK;
    if (!c->d_hints)
    {
        const size_t bytes = local_pixels(c) * sizeof(int) * OCCLUDER_HINTS;
        RT_HIP(c, hipMalloc(&c->d_hints, bytes));
        RT_HIP(c, hipMemset(c->d_hints, 0xff, bytes)); /* complete before any stream's launch below: once per context */
    }
    *hints = c->d_hints;
    return RT_OK;
}

/* one argument list for every form of k_generate_candidate: each takes all 14, S without its grid where the form has none */
struct GenArgs
{
    SceneViewGrid S;
    FrameParams P;
    const float4 *g0, *g1, *prev_rec, *prev_rad;
    float4 *out_rec, *out_rad;
    uint32_t* vis_queue;
    unsigned int* vis_count;
    float4 *vis_w, *g0_w, *g1_w;
    int* hints;
};
extern "C++" { /* templates cannot live inside extern "C" */
/* row I of GEN_FORMS, if it is the wanted form: the statement that instantiates a form is the one that launches it */
template <size_t I> static bool launch_gen_row(const GenForm& want, const GenArgs& A, int g, hipStream_t s)
{
    constexpr GenForm F = GEN_FORMS[I];
    if (!(F == want)) return false;
    if constexpr (F.grid)
        k_generate_candidate<F.fuse, F.shadowed, F.defer, F.pipe, F.ws, F.raycast, F.power, F.reproject, F.motion, F.grid><<<g, TRACE_BLOCK, 0, s>>>(
            A.S, A.P, A.g0, A.g1, A.prev_rec, A.prev_rad, A.out_rec, A.out_rad, A.vis_queue, A.vis_count, A.vis_w, A.g0_w, A.g1_w, A.hints);
    else
        k_generate_candidate<F.fuse, F.shadowed, F.defer, F.pipe, F.ws, F.raycast, F.power, F.reproject, F.motion, F.grid><<<g, TRACE_BLOCK, 0, s>>>(
            static_cast<const SceneView&>(A.S), A.P, A.g0, A.g1, A.prev_rec, A.prev_rad, A.out_rec, A.out_rad, A.vis_queue, A.vis_count, A.vis_w, A.g0_w, A.g1_w, A.hints);
    return true;
}
template <size_t... I> static bool launch_gen_form(const GenForm& want, const GenArgs& A, int g, hipStream_t s, std::index_sequence<I...>)
{
    return (... || launch_gen_row<I>(want, A, g, s));
}
} /* extern "C++" */

/* staged: a launch of the staged frame (its stage 0 or the look-ahead's): the product's kernel then gets the context's occluder hints */
static int launch_generate(rt_ctx* c, const Launch& L, int frame, int dst_phys, int prev_phys, bool fuse, float4* raycast_vis, bool staged)
{
    GenArgs A = {};
    A.P = make_params(c, L, frame, 0, K_GENERATE);
    const int g = trace_grid(c, L);
    Stage0Inputs in = {};
    in.no_lights = c->n_lights == 0; in.ris = c->opt.ris_sample_count > 0;
    in.grid_on = c->grid_cells > 0; in.grid_ok = c->grid_built && c->h_grid.ok;
    in.power_on = c->light_mode == RT_LIGHTS_POWER; in.alias_ok = c->alias_ok;
    in.shadowed = c->opt.use_shadowed_target_function; in.fuse = fuse;
    /* before the tag below: dst may not be prev, but the order costs nothing. A motion launch is a reprojecting one */
    in.history_motion = fuse && history_motion(c, prev_phys, A.P, L.vis);
    in.history_camera = fuse && !in.history_motion && history_camera(c, prev_phys, A.P);
    in.temporal_unbiased = c->temporal_unbiased; in.defer_vis = c->tune_defer_vis; in.ris_pipe = c->tune_ris_pipe;
    in.ws = use_ws(c, g); in.raycast = raycast_vis != nullptr;
    const Stage0Plan plan = stage0_plan(in); /* every refusal before the first side effect */
    if (plan.code != RT_OK) RT_FAIL(c, plan.code, "%s", FORM_MESSAGE[plan.why]);
    const GenForm& F = plan.form;
    int* hints = nullptr;
    if (staged) { const int rc = staged_hints(c, &hints); if (rc != RT_OK) return rc; }
    SceneView S = make_scene(c);
    if (plan.tables == LIGHTS_GRID) { S.lights = c->d_lights_grid; S.light_ke = c->d_light_ke_grid; }
    if (plan.tables == LIGHTS_POWER) { S.lights = c->d_lights_power; S.light_alias = c->d_alias; }
    static_cast<SceneView&>(A.S) = S;
    A.S.grid = GridView{c->h_grid.bounds(), c->h_grid.B, c->d_grid_cells, c->d_grid_cell_prob, c->d_grid_runs, c->d_grid_run_slots}; /* null while off */
    const FrameParams Pu = A.P; /* the merge's: the history buffer's camera */
    if (plan.unbiased_merge)
    {
        /* the product's fused form, whichever the tuning picks, made to merge nothing: the reprojecting instantiation under a history
         * camera of NaNs. The fused kernels merge by template, not by FrameParams::use_temporal, so the NaN camera alone does it: the
         * launch still projects, draws and runs the rejection heuristics per pixel, but every gather fails the float range test
         * (temporal_reproject.h) and the merge sees Reservoir{}: weight 0 is never accepted, M + 0, and ucw is recomputed by the
         * expression that made it, so what the launch stores is the candidates' records bit for bit, each with its own
         * visibility-reuse ray walked. No instantiation changes and none is added to k_generate_candidate. The launch counts its
         * shaded pixels as merged by a reprojecting launch, without a valid history (rt_temporal_reprojection_stats); the merge
         * below adds the valid and the moved ones and does not count the pixels again. */
        const float qnan = __builtin_nanf("");
        A.P.prev_origin = A.P.prev_right = A.P.prev_up = F3(qnan, qnan, qnan);
    }
    tag_reservoir(c, dst_phys);
    /* the primary rays' form writes the G-buffer it does not read; the occluder hints are the work-sharing forms' */
    A.g0 = F.raycast ? nullptr : L.g0; A.g1 = F.raycast ? nullptr : L.g1;
    A.prev_rec = fuse ? c->d_rec[prev_phys] : nullptr; A.prev_rad = fuse ? c->d_rad[prev_phys] : nullptr;
    A.out_rec = c->d_rec[dst_phys]; A.out_rad = c->d_rad[dst_phys];
    if (F.raycast) { A.vis_w = raycast_vis; A.g0_w = L.g0; A.g1_w = L.g1; }
    A.hints = F.ws ? hints : nullptr;
#ifdef RT_EXPERIMENTS
    const int lane = (L.stream == c->aux_stream) ? 1 : 0;
    if (plan.deferred_queue)
    {
        /* fused + unshadowed: the visibility-reuse rays that survive the temporal merge go through a queue */
        const size_t npx = local_pixels(c);
        if (!c->d_visq[0])
        {
            RT_HIP(c, hipMalloc(&c->d_visq[0], npx * 4));
            RT_HIP(c, hipMalloc(&c->d_visq[1], npx * 4));
            RT_HIP(c, hipMalloc(&c->d_visq_count, 8));
            RT_HIP(c, hipMemsetAsync(c->d_visq_count, 0, 8, L.stream));
            RT_HIP(c, hipHostMalloc(&c->h_visq_count, 8, hipHostMallocDefault));
            c->h_visq_count[0] = c->h_visq_count[1] = 0xffffffffu;
        }
        if (c->visq_epoch != c->epoch) { c->h_visq_count[0] = c->h_visq_count[1] = 0xffffffffu; c->visq_epoch = c->epoch; }
        RT_HIP(c, hipMemsetAsync(c->d_visq_count + lane, 0, 4, L.stream));
        A.vis_queue = c->d_visq[lane]; A.vis_count = c->d_visq_count + lane;
    }
#endif
    if (!launch_gen_form(F, A, g, L.stream, std::make_index_sequence<GEN_FORM_COUNT>()))
        RT_FAIL(c, RT_ERR_STATE, "k_generate_candidate<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d> is not a row of GEN_FORMS (stage0_forms.h)", F.fuse,
                F.shadowed, F.defer, F.pipe, F.ws, F.raycast, F.power, F.reproject, F.motion, F.grid);
    RT_HIP(c, hipGetLastError());
#ifdef RT_EXPERIMENTS
    if (plan.deferred_queue)
    {
        /* grid of the walk: one queue entry per lane if the count is like the last one that reached the host (+50 %),
         * every pixel of the launch if that is unknown (first frame, camera / option change); the kernel's stride loop
         * covers any count */
        const unsigned int last = c->h_visq_count[lane];
        int gv = g;
        if (last != 0xffffffffu)
        {
            const unsigned long long want = ((unsigned long long)last * 3ull / 2ull + TRACE_BLOCK - 1) / TRACE_BLOCK + 64ull;
            gv = want < (unsigned long long)g ? (int)want : g;
        }
        k_candidate_visibility<<<gv, TRACE_BLOCK, 0, L.stream>>>(S, L.g0, L.g1, A.out_rec, c->d_visq[lane], c->d_visq_count + lane);
        RT_HIP(c, hipGetLastError());
        RT_HIP(c, hipMemcpyAsync(c->h_visq_count + lane, c->d_visq_count + lane, 4, hipMemcpyDeviceToHost, L.stream));
    }
#endif
    if (plan.unbiased_merge)
    {
        /* same stream, same rows, same tag: reads the G-buffer the launch above read or wrote, merges the history in place */
        k_temporal_unbiased<<<g, TRACE_BLOCK, 0, L.stream>>>(S, Pu, L.g0, L.g1, A.prev_rec, A.prev_rad, A.out_rec, A.out_rad, 0 /* the launch above has counted the merged pixels */);
        RT_HIP(c, hipGetLastError());
    }
    return RT_OK;
}

int rt_generate_candidate(rt_ctx* c, int frame, int dst)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    NEED_SCENE(c);
    NEED_RES(c, dst);
    ++c->res_epoch; /* a reservoir buffer changes outside the staged frame: a pipelined stage 0 is stale */
    if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "no G-buffer: call rt_raycast or upload RT_BUF_VISIBILITY first");
    return launch_generate(c, whole_launch(c), frame, c->frame.res_map[dst], 0, false);
}

extern "C++" {
/* row I of TEMPORAL_FORMS, if it is the wanted form (as launch_gen_row) */
template <size_t I> static bool launch_temporal_row(rt_ctx* c, const TemporalForm& want, const SceneView& S, const FrameParams& P, const Launch& L, int pp, int pi)
{
    constexpr TemporalForm F = TEMPORAL_FORMS[I];
    if (!(F == want)) return false;
    k_temporal<F.shadowed, F.reproject, F.motion><<<launch_grid(c, L), BLOCK, 0, c->stream>>>(S, P, c->gbuf.g0, c->gbuf.g1, c->d_rec[pp], c->d_rad[pp], c->d_rec[pi], c->d_rad[pi]);
    return true;
}
template <size_t... I>
static bool launch_temporal_form(rt_ctx* c, const TemporalForm& want, const SceneView& S, const FrameParams& P, const Launch& L, int pp, int pi, std::index_sequence<I...>)
{
    return (... || launch_temporal_row<I>(c, want, S, P, L, pp, pi));
}
} /* extern "C++" */

int rt_temporal_resampling(rt_ctx* c, int frame, int prev, int inout)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    NEED_SCENE(c);
    NEED_RES(c, prev);
    NEED_RES(c, inout);
    ++c->res_epoch; /* a reservoir buffer changes outside the staged frame: a pipelined stage 0 is stale */
    if (prev == inout) RT_FAIL(c, RT_ERR_ARG, "prev and inout must differ");
    const SceneView S = make_scene(c);
    const Launch L = whole_launch(c);
    FrameParams P = make_params(c, L, frame, 0);
    const int pp = c->frame.res_map[prev], pi = c->frame.res_map[inout];
    TemporalInputs in = {};
    in.shadowed = c->opt.use_shadowed_target_function; in.temporal_unbiased = c->temporal_unbiased;
    in.history_motion = history_motion(c, pp, P, c->gbuf.vis);
    in.history_camera = !in.history_motion && history_camera(c, pp, P);
    const TemporalPlan plan = temporal_plan(in);
    if (plan.code != RT_OK) RT_FAIL(c, plan.code, "%s", FORM_MESSAGE[plan.why]);
    tag_reservoir(c, pi, c->res_tag[pi].gserial); /* merged in place: its shaded bits stay those of the G-buffer it was made from */
    if (plan.unbiased_merge) /* rt_temporal_unbiased: the 1/Z merge wherever the history is gathered by reprojection */
    {
        P = make_params(c, L, frame, 0, K_GENERATE); /* a tracing kernel on 8 x 8 tiles: the candidates' tile order */
        history_camera(c, pp, P);
        k_temporal_unbiased<<<trace_grid(c, L), TRACE_BLOCK, 0, c->stream>>>(S, P, c->gbuf.g0, c->gbuf.g1, c->d_rec[pp], c->d_rad[pp], c->d_rec[pi], c->d_rad[pi], 1);
    }
    else if (!launch_temporal_form(c, plan.form, S, P, L, pp, pi, std::make_index_sequence<sizeof(TEMPORAL_FORMS) / sizeof(TemporalForm)>()))
        RT_FAIL(c, RT_ERR_STATE, "k_temporal<%d, %d, %d> is not a row of TEMPORAL_FORMS (stage0_forms.h)", plan.form.shadowed, plan.form.reproject, plan.form.motion);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

/* examples/10_restir_di/10_restir_di.cu:239-254: a plain copy of the owned rows */
int rt_save_temporal_reservoir(rt_ctx* c, int src, int dst)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    NEED_RES(c, src);
    NEED_RES(c, dst);
    ++c->res_epoch; /* a reservoir buffer changes outside the staged frame: a pipelined stage 0 is stale */
    if (src == dst) return RT_OK;
    const size_t off = (size_t)(c->row_begin - c->lrow0) * c->W;
    const size_t n = (size_t)(c->row_end - c->row_begin) * c->W;
    const int ps = c->frame.res_map[src], pd = c->frame.res_map[dst];
    c->res_tag[pd] = c->res_tag[ps];
    RT_HIP(c, hipMemcpyAsync(c->d_rec[pd] + 4 * off, c->d_rec[ps] + 4 * off, n * 64, hipMemcpyDeviceToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(c->d_rad[pd] + off, c->d_rad[ps] + off, n * 16, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}

/* rows a strip must hold beyond its own for spatial_resampling to be exact: the Gaussian offset is
 * bounded by radius/1.96 * sqrt(2*23*ln 2) because rv0 >= 2^-23 when non-zero */
static int halo_rows_needed(const rt_options& o)
{
    if (!o.use_spatial_resampling || o.spatial_resampling_sample_count <= 0) return 0;
    return (int)ceilf(o.spatial_resampling_radius / 1.96f * 5.6471f);
}
#ifndef RT_FUSE_FINAL_AUTO
#define RT_FUSE_FINAL_AUTO 0 /* what rt_tuning key 23 = -1 means for a whole-frame context, until measured */
#endif
#ifndef RT_SHADOWED_SPATIAL_LDS
#define RT_SHADOWED_SPATIAL_LDS 0 /* the walk's own LDS stack already limits the shadowed variant to 6 workgroups per CU */
#endif
/* the LDS-staged variant covers the default reach (87 px) and up to 5 neighbours. Whole-frame contexts only: the
 * kernel itself handles strips (tile origins by row range, halo rows' bits from the neighbours' flags), but there it is
 * no faster than the gather kernel (A/B r02: 0.517 / 0.517 ms per frame at 1080p in 8 strips, 1.308 / 1.289 at 4K) and
 * it adds the bitmap launch to every frame */
static bool use_lds_spatial(const rt_ctx* c)
{
    return (c->tune_spatial_variant == 1 || c->tune_spatial_variant == 3) && c->opt.use_spatial_resampling && !c->opt.use_shadowed_target_function &&
           !c->spatial_unbiased &&
           halo_rows_needed(c->opt) <= SPL_HALO && c->opt.spatial_resampling_sample_count <= 5 &&
           whole_frame(c);
}
/* shaded bit per pixel of all local rows, rebuilt on the launch's stream when the G-buffer or the halo flags changed.
 * rt_frame_stage does this right behind the raycast, on the main stream, so that a stage's two lanes only read it. */
static int refresh_shaded_bits(rt_ctx* c, const Launch& L)
{
    if (!c->gbuf.shaded_bits_stale || !c->gbuf.valid || !use_lds_spatial(c)) return RT_OK;
    const int words = (c->W + 31) / 32;
    if (!c->d_shaded_bits) RT_HIP(c, hipMalloc(&c->d_shaded_bits, (size_t)c->lrows * words * 4));
    k_shaded_bitmap<<<dim3((c->W + 255) / 256, c->lrows), 256, 0, L.stream>>>(c->W, c->lrows, L.g1, c->d_shaded_bits);
    RT_HIP(c, hipGetLastError());
    c->gbuf.shaded_bits_stale = false;
    return RT_OK;
}
/* register budget of the gather kernel when rt_tuning key 9 is -1. xnack-any code (until late r02) wanted 4 wavefronts per
 * SIMD to keep the neighbour window in L2 (0.184 against 0.202 ms unbounded); the xnack- build is flat across 4 / 5 / 6 /
 * unbounded (0.170 / 0.169 / 0.168 / 0.170 ms), 6 a hair ahead */
#ifndef RT_SPATIAL_GATHER_AUTO_WAVES
#define RT_SPATIAL_GATHER_AUTO_WAVES 6
#endif
#ifndef RT_SPATIAL_PIPE_AUTO_WAVES
#define RT_SPATIAL_PIPE_AUTO_WAVES 5 /* 16 more registers in flight than k_spatial_coop (the staged record parts) */
#endif
/* r05, rt_tuning key 23: the frame's last spatial pass shades its pixels itself (k_spatial_resolve). auto = whole-frame contexts;
 * the unshadowed cooperative kernel only (the shadowed pass spends its time in its own rays). */
static bool use_fused_final(const rt_ctx* c)
{
#ifndef RT_EXPERIMENTS
    return false; /* k_spatial_resolve: measured slower (profiles/r05_fused_tail_ab.txt), experiments build only */
#endif
    const int want = c->tune_fuse_final < 0 ? (whole_frame(c) ? RT_FUSE_FINAL_AUTO : 0) : c->tune_fuse_final;
    return want != 0 && !c->opt.use_shadowed_target_function && c->opt.use_spatial_resampling && !c->spatial_unbiased && c->tune_spatial_variant == 2 && !c->tune_stream &&
           c->opt.spatial_resampling_passes >= 1 && c->indirect == 0 /* rt_indirect runs between resolve and tone mapping */;
}
/* rt_spatial_unbiased: does the 1/Z pass run for the current options, and can it? (with use_spatial_resampling = 0 the pass copies its
 * input in either mode) */
static bool unbiased_applies(const rt_ctx* c) { return c->spatial_unbiased && c->opt.use_spatial_resampling; }
static int unbiased_check(rt_ctx* c)
{
    if (!unbiased_applies(c)) return RT_OK;
    if (c->opt.use_shadowed_target_function)
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_spatial_unbiased: the shadowed target function is not built for the 1/Z pass");
    if (c->opt.spatial_resampling_sample_count > 5)
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_spatial_unbiased: %d neighbours per pass, the 1/Z pass takes at most 5", c->opt.spatial_resampling_sample_count);
    return RT_OK;
}
static int launch_spatial(rt_ctx* c, const Launch& L, int frame, int pass, int in_phys, int out_phys, bool fuse_final = false)
{
    { const int rc = unbiased_check(c); if (rc != RT_OK) return rc; }
    const int need = halo_rows_needed(c->opt);
    if ((c->row_begin > 0 && c->row_begin - c->lrow0 < (need < c->row_begin ? need : c->row_begin)) ||
        (c->row_end < c->H && c->lrow0 + c->lrows - c->row_end < (need < c->H - c->row_end ? need : c->H - c->row_end)))
        RT_FAIL(c, RT_ERR_STATE, "strip halo of %d rows is too small: spatial_resampling_radius %.1f needs %d", c->halo,
                c->opt.spatial_resampling_radius, need);
    const SceneView S = make_scene(c);
    const FrameParams P = make_params(c, L, frame, pass, K_SPATIAL);
    const bool lds_variant = use_lds_spatial(c);
    (void)lds_variant; /* the product build has no LDS-staged form */
    tag_reservoir(c, out_phys); /* a pass's output lies on the current camera's pixels (the history is never a pass's output) */
    if (unbiased_applies(c))
        /* one kernel whatever keys 8 and 23 say: the A/B forms restate the reference's pass */
        k_spatial_unbiased<<<trace_grid(c, L), TRACE_BLOCK, 0, L.stream>>>(S, P, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys]);
    else if (c->opt.use_shadowed_target_function)
    {
        /* the cooperative record traffic of key 8 = 2 applies to the <= 5 neighbour form (spatial_wave_shadowed) */
        if (c->tune_spatial_variant >= 2 && c->opt.use_spatial_resampling && c->opt.spatial_resampling_sample_count <= 5)
            k_spatial<true, true><<<trace_grid(c, L), TRACE_BLOCK, (size_t)(RT_SHADOWED_SPATIAL_LDS), L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys]);
        else
            k_spatial<true, false><<<trace_grid(c, L), TRACE_BLOCK, (size_t)(RT_SHADOWED_SPATIAL_LDS), L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys]);
    }
#ifdef RT_EXPERIMENTS
    else if (lds_variant && c->tune_spatial_variant == 3)
    {
        /* software-pipelined cooperative kernel (r04): staged shaded bits + the next neighbour's record in flight */
        const int rc = refresh_shaded_bits(c, L);
        if (rc != RT_OK) return rc;
#define RT_SPP(WV) k_spatial_pipe<WV><<<launch_grid(c, L), BLOCK, (size_t)c->tune_spatial_lds, L.stream>>>(P, c->d_shaded_bits, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys])
        switch (c->tune_spatial_waves < 0 ? RT_SPATIAL_PIPE_AUTO_WAVES : c->tune_spatial_waves) { case 4: RT_SPP(4); break; case 5: RT_SPP(5); break; case 6: RT_SPP(6); break; default: RT_SPP(0); break; }
#undef RT_SPP
    }
    else if (lds_variant)
    {
        const int rc = refresh_shaded_bits(c, L); /* no-op inside rt_frame / rt_frame_stage: done behind the raycast */
        if (rc != RT_OK) return rc;
#define RT_SPL(WV) k_spatial_lds<WV><<<launch_grid(c, L), BLOCK, (size_t)c->tune_spatial_lds, L.stream>>>(P, c->d_shaded_bits, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys])
        switch (c->tune_spatial_waves) { case 4: RT_SPL(4); break; case 5: RT_SPL(5); break; case 6: RT_SPL(6); break; default: RT_SPL(0); break; }
#undef RT_SPL
    }
#endif
#ifdef RT_EXPERIMENTS
    else if (fuse_final)
    {
        /* the last pass + resolve (+ tone mapping) of the staged frame in one launch of one-wavefront workgroups */
        const bool fused = c->fuse.recv[0] || c->fuse.recv[1] || c->fuse.send[0] || c->fuse.send[1];
        const bool store = c->tune_fuse_final != 2; /* 2: A/B only, the pass's output buffer is NOT written */
        uint32_t* px = c->tune_fuse_tonemap ? (uint32_t*)c->d_pixels : nullptr;
#define RT_SPR(FU, ST) k_spatial_resolve<FU, ST><<<trace_grid(c, L), TRACE_BLOCK, 0, L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys], c->d_accum, px)
        if (fused) { if (store) RT_SPR(true, true); else RT_SPR(true, false); }
        else { if (store) RT_SPR(false, true); else RT_SPR(false, false); }
#undef RT_SPR
        c->frame.final_fused = true;
    }
#endif
#ifdef RT_EXPERIMENTS
    else if (c->tune_spatial_variant == 4)
    {
        /* r05, A/B only: k_spatial_coop as one-wavefront workgroups on 8 x 8 tiles (a finished wavefront's slot is refilled at once; a
         * 256-thread workgroup's four slots wait for four free slots on one CU: 5 400 of 6 144 slots filled on average). More
         * wavefronts in flight (5 750), each slower (25.9 -> 27.9 us): the pass is bound by its misses in flight, +1.3 % */
        const bool fused = c->fuse.recv[0] || c->fuse.recv[1] || c->fuse.send[0] || c->fuse.send[1];
#define RT_SPC1(FU) k_spatial_coop<RT_SPATIAL_GATHER_AUTO_WAVES, FU, TRACE_BLOCK><<<trace_grid(c, L), TRACE_BLOCK, (size_t)c->tune_spatial_lds, L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys])
        if (fused) RT_SPC1(true); else RT_SPC1(false);
#undef RT_SPC1
    }
#endif
    else if (c->tune_spatial_variant == 2 || c->tune_spatial_variant == 3) /* 3 where the pipelined kernel does not apply (strips, radius > 30, > 5 neighbours) */
    {
#define RT_SPC2(WV, FU) k_spatial_coop<WV, FU><<<launch_grid(c, L), BLOCK, (size_t)c->tune_spatial_lds, L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys])
#define RT_SPC(WV) do { if (fused) RT_SPC2(WV, true); else RT_SPC2(WV, false); } while (0)
        const bool fused = c->fuse.recv[0] || c->fuse.recv[1] || c->fuse.send[0] || c->fuse.send[1];
#ifdef RT_EXPERIMENTS
        switch (c->tune_spatial_waves < 0 ? RT_SPATIAL_GATHER_AUTO_WAVES : c->tune_spatial_waves) { case 4: RT_SPC(4); break; case 5: RT_SPC(5); break; case 6: RT_SPC(6); break; default: RT_SPC(0); break; }
#else
        RT_SPC(RT_SPATIAL_GATHER_AUTO_WAVES); /* the product library carries the one register budget it uses (rt_tuning key 9: experiments build) */
#endif
#undef RT_SPC2
#undef RT_SPC
    }
#ifdef RT_EXPERIMENTS
    else
    {
#define RT_SPG(WV) k_spatial_gather<WV><<<launch_grid(c, L), BLOCK, (size_t)c->tune_spatial_lds, L.stream>>>(S, P, c->fuse, L.g0, L.g1, c->d_rec[in_phys], c->d_rad[in_phys], c->d_rec[out_phys], c->d_rad[out_phys])
        switch (c->tune_spatial_waves < 0 ? RT_SPATIAL_GATHER_AUTO_WAVES : c->tune_spatial_waves) { case 4: RT_SPG(4); break; case 5: RT_SPG(5); break; case 6: RT_SPG(6); break; default: RT_SPG(0); break; }
#undef RT_SPG
    }
#else
    else RT_FAIL(c, RT_ERR_UNSUPPORTED, "spatial variant %d is an A/B form of librestir_rt_exp.so", c->tune_spatial_variant);
#endif
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

int rt_spatial_resampling(rt_ctx* c, int frame, int pass, int in, int out)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    NEED_SCENE(c);
    NEED_RES(c, in);
    NEED_RES(c, out);
    ++c->res_epoch; /* a reservoir buffer changes outside the staged frame: a pipelined stage 0 is stale */
    if (in == out) RT_FAIL(c, RT_ERR_ARG, "in and out must differ");
    c->last_frame = frame;
    c->fuse = HaloFuse{};
    if (c->res_tag[c->frame.res_map[in]].gserial != c->gbuf.serial)
    {
        /* the G-buffer changed since `in` was written: its neighbour test must see the current shaded flags (frame_kernels.h) */
        /* own rows always; a strip's halo rows only where the neighbour's flags in g1 are of the current epoch (rt_halo_flags_unpack
         * after the last camera / scene / option change): stale flags must not rewrite the bits of the neighbour's records */
        const int first_row = (c->row_begin > c->lrow0 && c->halo_flags_epoch[0] != c->epoch) ? c->row_begin : c->lrow0;
        const int last_row = (c->lrow0 + c->lrows > c->row_end && c->halo_flags_epoch[1] != c->epoch) ? c->row_end : c->lrow0 + c->lrows;
        const size_t off = (size_t)(first_row - c->lrow0) * c->W;
        const int n = (last_row - first_row) * c->W;
        k_refresh_shaded<<<(n + 255) / 256, 256, 0, c->stream>>>(n, c->gbuf.g1 + off, c->d_rec[c->frame.res_map[in]] + 4 * off);
        RT_HIP(c, hipGetLastError());
        c->res_tag[c->frame.res_map[in]].gserial = c->gbuf.serial;
    }
    return launch_spatial(c, whole_launch(c), frame, pass, c->frame.res_map[in], c->frame.res_map[out]);
}

/* pixels: the staged frame maps each pixel in the resolve kernel itself (rt_tuning key 20, default on); NULL = resolve alone */
static int launch_resolve(rt_ctx* c, const Launch& L, int phys, uint32_t* pixels = nullptr)
{
    const int g = trace_grid(c, L);
#ifdef RT_EXPERIMENTS
    if (c->tune_stream)
    {
        /* persistent wavefronts, tiles dealt out round-robin (no job counter) */
        const int resident = c->n_cus * 4 * RT_RESOLVE_STREAM_WAVES; /* wavefronts the GPU holds at once: a multiple of 8 */
        const int wgs = g < resident ? g : resident;
        k_resolve_stream<<<wgs, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), make_params(c, L, 0, 0, K_RESOLVE), L.g0, L.g1, c->d_rec[phys], c->d_rad[phys], c->d_accum, g);
    }
    else
#endif
    if (use_ws(c, g)) k_resolve<true><<<g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), make_params(c, L, 0, 0, K_RESOLVE), L.g0, L.g1, c->d_rec[phys], c->d_rad[phys], c->d_accum, pixels);
    else k_resolve<false><<<g, TRACE_BLOCK, 0, L.stream>>>(make_scene(c), make_params(c, L, 0, 0, K_RESOLVE), L.g0, L.g1, c->d_rec[phys], c->d_rad[phys], c->d_accum, pixels);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_resolve(rt_ctx* c, int res)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    NEED_SCENE(c);
    NEED_RES(c, res);
    return launch_resolve(c, whole_launch(c), c->frame.res_map[res]);
}

static int launch_tone_mapping(rt_ctx* c, const Launch& L)
{
    k_tone_mapping<<<launch_grid(c, L), BLOCK, 0, L.stream>>>(make_params(c, L, 0, 0), c->d_accum, c->d_pixels);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_tone_mapping(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    return launch_tone_mapping(c, whole_launch(c));
}

/* kernelMain of examples/04_ao/04_ao.cu:31-88 = 06_ao_hiprt.cu:35-91 (frame_kernels.h k_ao): RGBA8 straight into the pixel
 * buffer over the context's own rows; the accumulation buffer, the frame number and the options play no part */
static int launch_ao(rt_ctx* c)
{
    const SceneView S = make_scene(c);
    const Launch L = whole_launch(c);
    const FrameParams P = make_params(c, L, 0, 0, K_RAYCAST); /* the tracing kernels' tile order: interleaved over the XCDs */
    const int g = trace_grid(c, L);
    RT_HIP(c, hipMemsetAsync(c->d_counter, 0, 8, c->stream));
    if (c->tune_ao_layout == 1) k_ao<1><<<g, TRACE_BLOCK, 0, c->stream>>>(S, P, c->d_pixels, c->d_counter);
    else k_ao<0><<<g, TRACE_BLOCK, 0, c->stream>>>(S, P, c->d_pixels, c->d_counter);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

/* `path_trace` of examples/07_pt/07_pt.cu (example 7), examples/08_nee/08_nee.cu (8) or examples/09_ris/09_ris.cu (9);
 * example 4 / 6: the ambient occlusion of examples/04_ao/04_ao.cu / examples/06_ao_hiprt/06_ao_hiprt.cu (launch_ao) */
int rt_path_trace(rt_ctx* c, int example, int frame)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    NEED_SCENE(c);
    if (example == 4 || example == 6) return launch_ao(c);
    if (example != 7 && example != 8 && example != 9) RT_FAIL(c, RT_ERR_ARG, "example must be 4 (04_ao), 6 (06_ao_hiprt), 7 (07_pt), 8 (08_nee) or 9 (09_ris)");
    if (example != 7 && c->n_lights == 0) RT_FAIL(c, RT_ERR_STATE, "08_nee / 09_ris need at least one emissive triangle");
    const SceneView S = make_scene(c);
    const Launch L = whole_launch(c);
    FrameParams P = make_params(c, L, frame, 0, K_RAYCAST);
    const f3 sky = F3(c->opt.sky_color[0], c->opt.sky_color[1], c->opt.sky_color[2]);
    const int g = trace_grid(c, L);
    const int md = c->opt.max_depth;
    const bool sh = c->opt.use_shadowed_target_function != 0;
    const bool wavefront = c->pt_wavefront == 1 || (c->pt_wavefront == 2 && example == 9);
    /* one launch per bounce: the first launch's tile order is the order of the path list every later bounce walks — an XCD's
     * band of the image keeps neighbouring paths on one XCD (interleaved: +2 %); one launch per frame gains 5-10 % interleaved
     * like the frame's tracing kernels (profiles/r05_tile_interleave_ab.txt) */
    if (wavefront && c->tune_tile_mode[K_RAYCAST] < 0) P.tile_mode = 1;
    if (wavefront && md > 0 && md <= 60)
    {
        /* one launch per bounce over the compacted list of live paths */
        const size_t n = (size_t)c->W * (size_t)(c->row_end - c->row_begin);
        if (!c->d_paths[0])
        {
            RT_HIP(c, hipMalloc(&c->d_paths[0], n * 64));
            RT_HIP(c, hipMalloc(&c->d_paths[1], n * 64));
            RT_HIP(c, hipMalloc(&c->d_pt_counters, 64 * 8));
        }
        RT_HIP(c, hipMemsetAsync(c->d_pt_counters, 0, 64 * 8, c->stream));
        k_pt_init<<<g, TRACE_BLOCK, 0, c->stream>>>(P, c->d_paths[0], c->d_pt_counters);
        RT_HIP(c, hipGetLastError());
        const int gb = (int)((n + TRACE_BLOCK - 1) / TRACE_BLOCK);
        for (int d = 0; d < md; ++d)
        {
            const float4* in = c->d_paths[d & 1];
            float4* out = c->d_paths[(d + 1) & 1];
            if (example == 7) k_pt_bounce<7, false><<<gb, TRACE_BLOCK, 0, c->stream>>>(S, P, d, md, sky, in, out, c->d_accum, c->d_pt_counters);
            else if (example == 8) k_pt_bounce<8, false><<<gb, TRACE_BLOCK, 0, c->stream>>>(S, P, d, md, sky, in, out, c->d_accum, c->d_pt_counters);
            else if (sh) k_pt_bounce<9, true><<<gb, TRACE_BLOCK, 0, c->stream>>>(S, P, d, md, sky, in, out, c->d_accum, c->d_pt_counters);
            else k_pt_bounce<9, false><<<gb, TRACE_BLOCK, 0, c->stream>>>(S, P, d, md, sky, in, out, c->d_accum, c->d_pt_counters);
            RT_HIP(c, hipGetLastError());
        }
        RT_HIP(c, hipMemcpyAsync(c->d_counter, c->d_pt_counters, 8, hipMemcpyDeviceToDevice, c->stream));
        return RT_OK;
    }
    RT_HIP(c, hipMemsetAsync(c->d_counter, 0, 8, c->stream));
    if (example == 7) k_path_trace<7, false><<<launch_grid(c, L), BLOCK, 0, c->stream>>>(S, P, md, sky, c->d_accum, c->d_counter);
    else if (example == 8) k_path_trace<8, false><<<g, TRACE_BLOCK, 0, c->stream>>>(S, P, md, sky, c->d_accum, c->d_counter);
    else if (sh) k_path_trace<9, true><<<g, TRACE_BLOCK, 0, c->stream>>>(S, P, md, sky, c->d_accum, c->d_counter);
    else k_path_trace<9, false><<<g, TRACE_BLOCK, 0, c->stream>>>(S, P, md, sky, c->d_accum, c->d_counter);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
/* raytrace() calls made by the last rt_path_trace (synchronises the stream) */
int rt_path_trace_rays(rt_ctx* c, uint64_t* rays)
{
    RT_CHECK_CTX(c);
    if (!rays) return RT_ERR_ARG;
    unsigned long long h = 0;
    RT_HIP(c, hipMemcpyAsync(&h, c->d_counter, 8, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    *rays = h;
    return RT_OK;
}

/* ---- rt_indirect (indirect.h, frame_kernels.h k_indirect*) ---- */
static const char* const kNoLights = "08_nee / 09_ris need at least one emissive triangle";
/* the pass over the launch's rows, on its stream, reading ITS G-buffer set */
static int launch_indirect(rt_ctx* c, const Launch& L, int frame, int bounces)
{
    if (c->n_lights == 0) RT_FAIL(c, RT_ERR_STATE, "%s", kNoLights);
    if (!c->d_ind_counters) RT_HIP(c, hipMalloc(&c->d_ind_counters, 64 * 8));
    const bool timed = c->timing && L.timed;
    if (timed && !c->ind_ev[0]) for (auto& e : c->ind_ev) RT_HIP(c, hipEventCreate(&e));
    const SceneView S = make_scene(c);
    const FrameParams P = make_params(c, L, frame, 0, K_RAYCAST); /* the tracing kernels' tile order and its tuning key */
    const int g = trace_grid(c, L);
    if (timed) RT_HIP(c, hipEventRecord(c->ind_ev[0], L.stream));
    RT_HIP(c, hipMemsetAsync(c->d_ind_counters, 0, 64 * 8, L.stream));
    k_indirect<<<g, TRACE_BLOCK, 0, L.stream>>>(S, P, bounces, L.g0, L.g1, c->d_accum, c->d_ind_counters);
    RT_HIP(c, hipGetLastError());
    if (timed) RT_HIP(c, hipEventRecord(c->ind_ev[1], L.stream));
    c->ind_timed = timed;
    c->ind_bounces = bounces;
    return RT_OK;
}
int rt_indirect(rt_ctx* c, int bounces)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_indirect: strip contexts hold no path lists and their frame is the strip driver's (rows [%d,%d) of %d)", c->row_begin, c->row_end, c->H);
    if (bounces < 0 || bounces > 32) RT_FAIL(c, RT_ERR_ARG, "rt_indirect: bounces %d outside 0..32", bounces);
    c->indirect = bounces;
    ++c->epoch;
    return RT_OK;
}
int rt_indirect_get(rt_ctx* c, int* bounces)
{
    RT_CHECK_CTX(c);
    if (!bounces) return RT_ERR_ARG;
    *bounces = c->indirect;
    return RT_OK;
}
int rt_indirect_pass(rt_ctx* c, int frame, int bounces)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_indirect_pass is for whole-frame contexts (rows [%d,%d) of %d)", c->row_begin, c->row_end, c->H);
    JOIN_TAIL(c);
    NEED_SCENE(c);
    if (bounces < 1 || bounces > 32) RT_FAIL(c, RT_ERR_ARG, "rt_indirect_pass: bounces %d outside 1..32", bounces);
    if (!c->gbuf.valid || c->gbuf.traced_epoch != c->epoch)
        RT_FAIL(c, RT_ERR_STATE, "rt_indirect_pass: no traced G-buffer of the current camera and scene (rt_raycast or rt_frame first)");
    return launch_indirect(c, whole_launch(c), frame, bounces);
}
int rt_indirect_stats(rt_ctx* c, uint64_t out[3])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_ind_counters || c->ind_bounces < 1) RT_FAIL(c, RT_ERR_STATE, "rt_indirect_stats: no indirect pass has run");
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    unsigned long long h[64];
    RT_HIP(c, hipMemcpy(h, c->d_ind_counters, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[1]; out[1] = h[0]; out[2] = h[2 + c->ind_bounces];
    return RT_OK;
}
int rt_indirect_timing(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->ind_timed) RT_FAIL(c, RT_ERR_STATE, "no timed indirect pass (rt_timing_enable, then rt_indirect_pass or rt_frame with rt_indirect on)");
    RT_HIP(c, hipEventSynchronize(c->ind_ev[1]));
    RT_HIP(c, hipEventElapsedTime(ms, c->ind_ev[0], c->ind_ev[1]));
    return RT_OK;
}

/* ---- rt_denoise (denoise_kernels.h): guide, demodulation, variance, the a-trous levels; asynchronous on the context's stream ---- */
/* what rt_denoise and rt_denoise_temporal share: the checks, the buffers, the guide pass and one a-trous level */
static int denoise_begin(rt_ctx* c, const rt_denoise_params* params, rt_denoise_params& d, const char* name)
{
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "%s is for whole-frame contexts (rows [%d,%d) of %d)", name, c->row_begin, c->row_end, c->H);
    NEED_SCENE(c);
    d = rt_denoise_params{5, 4.0f, 1.0f, 7, 3};
    if (params) d = *params;
    if (d.iterations < 0 || d.iterations > 8) RT_FAIL(c, RT_ERR_ARG, "iterations %d outside 0..8", d.iterations);
    if (!(d.sigma_luminance > 0.0f) || !(d.sigma_luminance < INFINITY)) RT_FAIL(c, RT_ERR_ARG, "sigma_luminance must be finite and > 0");
    if (!(d.sigma_plane > 0.0f) || !(d.sigma_plane < INFINITY)) RT_FAIL(c, RT_ERR_ARG, "sigma_plane must be finite and > 0");
    if (d.normal_power_log2 < 0 || d.normal_power_log2 > 10) RT_FAIL(c, RT_ERR_ARG, "normal_power_log2 %d outside 0..10", d.normal_power_log2);
    if (d.variance_radius < 0 || d.variance_radius > 3) RT_FAIL(c, RT_ERR_ARG, "variance_radius %d outside 0..3", d.variance_radius);
    if (c->n_tris > (1 << 30)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "the guide word holds triangle indices below 2^30");
    return RT_OK;
}
static int denoise_alloc(rt_ctx* c)
{
    RT_HIP(c, hipSetDevice(c->device));
    const size_t n = local_pixels(c);
    if (!c->d_dn_hdr)
    {
        float4** bufs[6] = {&c->d_dn_vis, &c->d_dn_gx, &c->d_dn_gn, &c->d_dn_col[0], &c->d_dn_col[1], &c->d_dn_hdr};
        for (float4** b : bufs)
            if (!*b) RT_HIP(c, hipMalloc(b, n * 16));
    }
    return RT_OK;
}
static int denoise_guide(rt_ctx* c, const SceneView& S, hipStream_t st, float4* gx, float4* gn)
{
    const FrameParams PG = make_params(c, whole_launch(c), 0, 0, K_RAYCAST);
    const int g = trace_grid(c, whole_launch(c));
    if (use_ws_primary(c, g)) k_denoise_guide<true><<<g, TRACE_BLOCK, 0, st>>>(S, PG, c->d_dn_vis, gx, gn);
    else k_denoise_guide<false><<<g, TRACE_BLOCK, 0, st>>>(S, PG, c->d_dn_vis, gx, gn);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
/* a-trous level at `step` from cin into cout; the last level writes the HDR output and the pixels (and cout unless it is null) */
static int denoise_level(rt_ctx* c, const FrameParams& P, const DnParams& D, hipStream_t st, int step, bool last, const float4* gx,
                         const float4* gn, const float4* cin, float4* cout)
{
    if (c->tune_dn_layout == 1)
    {
        const int nbx = ((c->W + step - 1) / step + DN_LDS_BLOCK - 1) / DN_LDS_BLOCK, nby = ((c->H + step - 1) / step + DN_LDS_BLOCK - 1) / DN_LDS_BLOCK;
        const int gl = step * step * nbx * nby;
        if (last) k_denoise_iter_lds<true><<<gl, DN_LDS_BLOCK * DN_LDS_BLOCK, 0, st>>>(P, D, step, nbx, nby, c->d_trimat, c->d_accum, gx, gn, cin, cout, c->d_dn_hdr, c->d_pixels);
        else k_denoise_iter_lds<false><<<gl, DN_LDS_BLOCK * DN_LDS_BLOCK, 0, st>>>(P, D, step, nbx, nby, c->d_trimat, c->d_accum, gx, gn, cin, cout, nullptr, nullptr);
    }
    else if (last) k_denoise_iter<true><<<launch_grid(c, whole_launch(c)), BLOCK, 0, st>>>(P, D, step, c->d_trimat, c->d_accum, gx, gn, cin, cout, c->d_dn_hdr, c->d_pixels);
    else k_denoise_iter<false><<<launch_grid(c, whole_launch(c)), BLOCK, 0, st>>>(P, D, step, c->d_trimat, c->d_accum, gx, gn, cin, cout, nullptr, nullptr);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
#define DN_CK(x) do { const int _r = (x); if (_r != RT_OK) return _r; } while (0)

int rt_denoise(rt_ctx* c, const rt_denoise_params* params)
{
    RT_CHECK_CTX(c);
    rt_denoise_params d;
    DN_CK(denoise_begin(c, params, d, "rt_denoise"));
    DN_CK(denoise_alloc(c));
    /* what may still write the accumulation buffer (or the pixels): the previous frame's resolve + tone mapping on the tail stream,
     * the look-ahead stage 0 (waited for, not dropped: its results stay valid for the next frame). What comes after on this stream
     * is ordered behind the launches below; the next staged frame's tail forks from this stream behind them. */
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    hipStream_t st = c->stream;
    const bool timed = c->timing;
    if (timed && !c->dn_ev[0])
        for (auto& e : c->dn_ev) RT_HIP(c, hipEventCreate(&e));
    if (timed) RT_HIP(c, hipEventRecord(c->dn_ev[0], st));
    const SceneView S = make_scene(c);
    DN_CK(denoise_guide(c, S, st, c->d_dn_gx, c->d_dn_gn));
    if (timed) RT_HIP(c, hipEventRecord(c->dn_ev[1], st));
    const FrameParams P = make_params(c, whole_launch(c), 0, 0, K_SPATIAL);
    const DnParams D = {d.iterations, d.sigma_luminance, d.sigma_plane, d.normal_power_log2, d.variance_radius};
    const int g = launch_grid(c, whole_launch(c));
    k_denoise_demod<<<g, BLOCK, 0, st>>>(P, c->d_trimat, c->d_accum, c->d_dn_gn, c->d_dn_col[1]);
    k_denoise_var<<<g, BLOCK, 0, st>>>(P, D, c->d_dn_gx, c->d_dn_gn, c->d_dn_col[1], c->d_dn_col[0]);
    RT_HIP(c, hipGetLastError());
    if (timed) RT_HIP(c, hipEventRecord(c->dn_ev[2], st));
    if (d.iterations == 0)
    {
        if (timed) RT_HIP(c, hipEventRecord(c->dn_ev[3], st));
        k_denoise_output<<<g, BLOCK, 0, st>>>(P, c->d_trimat, c->d_accum, c->d_dn_gn, c->d_dn_col[0], c->d_dn_hdr, c->d_pixels);
    }
    for (int i = 0; i < d.iterations; ++i)
    {
        const bool last = i + 1 == d.iterations;
        if (timed && last) RT_HIP(c, hipEventRecord(c->dn_ev[3], st));
        DN_CK(denoise_level(c, P, D, st, 1 << i, last, c->d_dn_gx, c->d_dn_gn, c->d_dn_col[i & 1], last ? nullptr : c->d_dn_col[(i + 1) & 1]));
    }
    RT_HIP(c, hipGetLastError());
    if (timed) RT_HIP(c, hipEventRecord(c->dn_ev[4], st));
    c->dn_timed = timed;
    c->dn_valid = true;
    return RT_OK;
}
int rt_denoise_timing(rt_ctx* c, float ms[5])
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->dn_timed) RT_FAIL(c, RT_ERR_STATE, "no timed rt_denoise (rt_timing_enable + rt_denoise first)");
    RT_HIP(c, hipEventSynchronize(c->dn_ev[4]));
    for (int k = 0; k < 4; ++k) RT_HIP(c, hipEventElapsedTime(&ms[k], c->dn_ev[k], c->dn_ev[k + 1]));
    RT_HIP(c, hipEventElapsedTime(&ms[4], c->dn_ev[0], c->dn_ev[4]));
    return RT_OK;
}

/* ---- rt_denoise_temporal (denoise_kernels.h): guide, reprojection + integration, variance with history, rt_denoise's levels.
 * Buffers: k_denoise_temporal reads the previous guide / moments [1 - cur] and the colour history, writes the integrated colour
 * into d_dn_col[1] and the moments [cur]; k_denoise_var_hist -> d_dn_col[0] (0 iterations: d_dt_col, the history itself);
 * level 1 -> d_dt_col (it has been read already), level i >= 2 -> d_dn_col[i & 1]. ---- */
int rt_denoise_temporal(rt_ctx* c, const rt_denoise_params* spatial, const rt_denoise_temporal_params* temporal)
{
    RT_CHECK_CTX(c);
    rt_denoise_params d;
    DN_CK(denoise_begin(c, spatial, d, "rt_denoise_temporal"));
    rt_denoise_temporal_params t = {0.2f, 0.2f};
    if (temporal) t = *temporal;
    if (!(t.alpha_color > 0.0f && t.alpha_color <= 1.0f)) RT_FAIL(c, RT_ERR_ARG, "alpha_color must be in (0, 1]");
    if (!(t.alpha_moments > 0.0f && t.alpha_moments <= 1.0f)) RT_FAIL(c, RT_ERR_ARG, "alpha_moments must be in (0, 1]");
    DN_CK(denoise_alloc(c));
    const size_t n = local_pixels(c);
    if (!c->d_dt_col)
    {
        float4** bufs[7] = {&c->d_dt_gx[0], &c->d_dt_gx[1], &c->d_dt_gn[0], &c->d_dt_gn[1], &c->d_dt_mom[0], &c->d_dt_mom[1], &c->d_dt_col};
        for (float4** b : bufs)
            if (!*b) RT_HIP(c, hipMalloc(b, n * 16));
    }
    JOIN_TAIL(c); /* as rt_denoise */
    JOIN_SPEC(c);
    hipStream_t st = c->stream;
    const bool timed = c->timing;
    if (timed && !c->dt_ev[0])
        for (auto& e : c->dt_ev) RT_HIP(c, hipEventCreate(&e));
    const int cur = c->dt_valid ? 1 - c->dt_cur : c->dt_cur, prev = 1 - cur;
    if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[0], st));
    const SceneView S = make_scene(c);
    DN_CK(denoise_guide(c, S, st, c->d_dt_gx[cur], c->d_dt_gn[cur]));
    if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[1], st));
    const FrameParams P = make_params(c, whole_launch(c), 0, 0, K_SPATIAL);
    const DnParams D = {d.iterations, d.sigma_luminance, d.sigma_plane, d.normal_power_log2, d.variance_radius};
    DnTemporal T;
    unpack_camera(c->dt_tag.rg, T.rg_origin, T.rg_right, T.rg_up);
    T.alpha_c = t.alpha_color;
    T.alpha_m = t.alpha_moments;
    T.has_history = c->dt_valid ? 1 : 0;
    const int g = launch_grid(c, whole_launch(c));
    float4 *gx = c->d_dt_gx[cur], *gn = c->d_dt_gn[cur], *mom = c->d_dt_mom[cur];
    /* rt_denoise_temporal_motion: a history of exactly the generation d_tv_prev describes, which is not the current one */
    const bool followed = c->moved.follows(FOLLOW_DENOISER, c->dt_tag, c->dt_valid);
    /* rt_denoise_temporal_antilag: an adapted call gathers first and blends in k_denoise_antilag; any other call is the one it was */
    const bool adapted = c->al_on && c->dt_valid;
    DnMotion M = {};
    if (followed)
    {
        M.eye_prev = f3_of(c->dt_tag.eye);
        M.lo = c->moved.lo; M.hi = c->moved.hi;
        M.tv_prev = c->d_tv_prev;
        M.vis = c->d_dn_vis;
    }
    if (adapted)
    {
        const rt_denoise_antilag_params& a = c->al_params;
        const DnAntilag L = {a.radius, a.gradient_lo, a.gradient_hi, a.floor};
        if (followed)
            k_denoise_antilag_gather<true><<<g, BLOCK, 0, st>>>(P, T, M, c->d_trimat, c->d_accum, gx, gn, c->d_dt_gx[prev], c->d_dt_gn[prev], c->d_dt_col,
                                                                c->d_dt_mom[prev], c->d_dn_col[0], c->d_dn_col[1], mom);
        else
            k_denoise_antilag_gather<false><<<g, BLOCK, 0, st>>>(P, T, M, c->d_trimat, c->d_accum, gx, gn, c->d_dt_gx[prev], c->d_dt_gn[prev], c->d_dt_col,
                                                                 c->d_dt_mom[prev], c->d_dn_col[0], c->d_dn_col[1], mom);
        RT_HIP(c, hipGetLastError());
        if (timed)
        {
            if (!c->al_ev) RT_HIP(c, hipEventCreate(&c->al_ev));
            RT_HIP(c, hipEventRecord(c->al_ev, st));
        }
        const int ntx = (c->W + DN_AL_TILE_W - 1) / DN_AL_TILE_W, nty = (c->H + DN_AL_TILE_H - 1) / DN_AL_TILE_H;
        k_denoise_antilag<<<ntx * nty, DN_AL_THREADS, 0, st>>>(c->W, c->H, ntx, L, T.alpha_c, T.alpha_m, gn, c->d_dn_col[0], c->d_dn_col[1], mom);
    }
    else if (followed)
    {
        k_denoise_temporal_motion<<<g, BLOCK, 0, st>>>(P, T, M, c->d_trimat, c->d_accum, gx, gn, c->d_dt_gx[prev], c->d_dt_gn[prev], c->d_dt_col,
                                                       c->d_dt_mom[prev], c->d_dn_col[1], mom);
    }
    else
        k_denoise_temporal<<<g, BLOCK, 0, st>>>(P, T, c->d_trimat, c->d_accum, gx, gn, c->d_dt_gx[prev], c->d_dt_gn[prev], c->d_dt_col,
                                                c->d_dt_mom[prev], c->d_dn_col[1], mom);
    RT_HIP(c, hipGetLastError());
    if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[2], st));
    float4* var_out = d.iterations == 0 ? c->d_dt_col : c->d_dn_col[0];
    k_denoise_var_hist<<<g, BLOCK, 0, st>>>(P, D, gx, gn, mom, c->d_dn_col[1], var_out);
    RT_HIP(c, hipGetLastError());
    if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[3], st));
    if (d.iterations == 0)
    {
        if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[4], st));
        k_denoise_output<<<g, BLOCK, 0, st>>>(P, c->d_trimat, c->d_accum, gn, var_out, c->d_dn_hdr, c->d_pixels);
        RT_HIP(c, hipGetLastError());
    }
    for (int i = 0; i < d.iterations; ++i)
    {
        const bool last = i + 1 == d.iterations;
        if (timed && last) RT_HIP(c, hipEventRecord(c->dt_ev[4], st));
        const float4* cin = i == 0 ? c->d_dn_col[0] : i == 1 ? c->d_dt_col : c->d_dn_col[(i - 1) & 1];
        float4* cout = i == 0 ? c->d_dt_col : last ? nullptr : c->d_dn_col[i & 1];
        DN_CK(denoise_level(c, P, D, st, 1 << i, last, gx, gn, cin, cout));
    }
    if (timed) RT_HIP(c, hipEventRecord(c->dt_ev[5], st));
    c->dt_tag.write(c->rg, c->moved.geo_gen, c->eye, 0);
    c->moved.tagged(FOLLOW_DENOISER);
    c->dt_followed = followed;
    c->al_adapted = adapted;
    c->al_timed = timed && adapted;
    c->dt_cur = cur;
    c->dt_valid = true;
    c->dt_timed = timed;
    c->dn_valid = true;
    return RT_OK;
}
/* r25. rt_denoise_temporal's history follows triangles moved by rt_scene_update (denoise_motion.h). Changes
 * results, so not an rt_tuning key. Independent of rt_temporal_reprojection / rt_temporal_motion, with which it shares d_tv_prev: the
 * first of the two toggles going on allocates it as a copy of the current vertices with an empty range, the last going off frees it
 * (after the stream has drained: launches in flight may read it); a toggle going on while it exists leaves it and the range alone.
 * Touches neither rt_state_epoch nor the look-ahead nor any reservoir or history buffer. */
int rt_denoise_temporal_motion(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_denoise_temporal_motion: rt_denoise_temporal is for whole-frame contexts");
    RT_HIP(c, hipSetDevice(c->device));
    return kept_vertices_toggled(c, c->moved.toggle(FOLLOW_DENOISER, on != 0, scene_has_vertices(c)));
}
int rt_denoise_temporal_motion_get(rt_ctx* c, int* on, int* last_call_followed)
{
    RT_CHECK_CTX(c);
    if (!on && !last_call_followed) return RT_ERR_ARG;
    if (on) *on = c->moved.on[FOLLOW_DENOISER] ? 1 : 0;
    if (last_call_followed) *last_call_followed = c->dt_followed ? 1 : 0;
    return RT_OK;
}
/* r30. rt_denoise_temporal raises its blend factors where the current frame and the reprojected history disagree over a window
 * (denoise_antilag.h). Changes results, so not an rt_tuning key. Host state only: it reads the history
 * rt_denoise_temporal keeps anyway, so it touches neither rt_state_epoch nor the look-ahead nor any buffer, and needs no reset. */
int rt_denoise_temporal_antilag(rt_ctx* c, int on, const rt_denoise_antilag_params* params)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_denoise_temporal_antilag: rt_denoise_temporal is for whole-frame contexts");
    rt_denoise_antilag_params a = {4, 0.2f, 0.8f, 0.05f};
    if (params) a = *params;
    if (a.radius < 1 || a.radius > DN_ANTILAG_RADIUS_MAX) RT_FAIL(c, RT_ERR_ARG, "radius %d outside 1..%d", a.radius, DN_ANTILAG_RADIUS_MAX);
    if (!(a.gradient_lo >= 0.0f) || !(a.gradient_hi < INFINITY) || !(a.gradient_lo < a.gradient_hi))
        RT_FAIL(c, RT_ERR_ARG, "gradient_lo and gradient_hi must be finite with 0 <= lo < hi");
    if (!(a.floor >= 0.0f) || !(a.floor < INFINITY)) RT_FAIL(c, RT_ERR_ARG, "floor must be finite and >= 0");
    c->al_on = on != 0;
    c->al_params = a;
    return RT_OK;
}
int rt_denoise_temporal_antilag_get(rt_ctx* c, int* on, rt_denoise_antilag_params* params, int* last_call_adapted)
{
    RT_CHECK_CTX(c);
    if (!on && !params && !last_call_adapted) return RT_ERR_ARG;
    if (on) *on = c->al_on ? 1 : 0;
    if (params) *params = c->al_params;
    if (last_call_adapted) *last_call_adapted = c->al_adapted ? 1 : 0;
    return RT_OK;
}
int rt_denoise_temporal_antilag_timing(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->dt_timed || !c->al_timed) RT_FAIL(c, RT_ERR_STATE, "no timed adapted rt_denoise_temporal (rt_timing_enable + rt_denoise_temporal_antilag + a call with a history first)");
    RT_HIP(c, hipEventSynchronize(c->dt_ev[2]));
    RT_HIP(c, hipEventElapsedTime(ms, c->al_ev, c->dt_ev[2]));
    return RT_OK;
}
int rt_denoise_temporal_reset(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    c->dt_valid = false; /* the next call reads none of the previous buffers */
    return RT_OK;
}
int rt_denoise_temporal_timing(rt_ctx* c, float ms[6])
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->dt_timed) RT_FAIL(c, RT_ERR_STATE, "no timed rt_denoise_temporal (rt_timing_enable + rt_denoise_temporal first)");
    RT_HIP(c, hipEventSynchronize(c->dt_ev[5]));
    for (int k = 0; k < 5; ++k) RT_HIP(c, hipEventElapsedTime(&ms[k], c->dt_ev[k], c->dt_ev[k + 1]));
    RT_HIP(c, hipEventElapsedTime(&ms[5], c->dt_ev[0], c->dt_ev[5]));
    return RT_OK;
}

int rt_timing_enable(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (on && !c->ev_created)
    {
        for (auto& e : c->ev) RT_HIP(c, hipEventCreate(&e));
        c->ev_created = true;
    }
    c->timing = on != 0;
    c->last_valid = false;
    return RT_OK;
}

/* The frame as a sequence of stages, so that a strip context can exchange halos in between:
 *   stage 0            [clear] raycast, generate_candidate(+temporal) into the rotating buffers
 *   stage 1..passes    spatial pass stage-1      (its input buffer must have valid halos)
 *   stage passes+1     resolve, tone_mapping, buffer renaming
 * rt_frame runs them back to back. */
/* begin: buffer roles of the stage; run: its kernels over storage rows [row0,row1) of the owned
 * rows (several runs per stage allowed: boundary rows first, interior later, so that halos can
 * travel while the interior is computed); end: advance. */
int rt_frame_stage_begin(rt_ctx* c, int frame, int stage, int clear_first)
{
    RT_CHECK_CTX(c);
    NEED_SCENE(c);
    if (stage == 0 && c->opt.spatial_resampling_passes > 0) { const int rc = unbiased_check(c); if (rc != RT_OK) return rc; } /* before the frame starts */
    if (stage == 0 && c->indirect > 0 && c->n_lights == 0) RT_FAIL(c, RT_ERR_STATE, "%s", kNoLights); /* rt_indirect: likewise */
    c->last_frame = frame;
    /* a spatial stage reads the shaded-bit rows from both lanes: (re)built here, on the main stream, if the halo flags
     * arrived after the raycast (cold frame of a strip) */
    if (stage >= 1) { const int rc = refresh_shaded_bits(c, whole_launch(c)); if (rc != RT_OK) return rc; }
    RT_HIP(c, hipEventRecord(c->ev_stage, c->stream)); /* everything the stage reads is complete here */
    c->aux_used = false;
    c->fuse = HaloFuse{};
    const int passes = c->opt.spatial_resampling_passes;
    if (stage == 0)
    {
        roles_begin(c->frame);
        c->frame.clear = clear_first != 0;
        c->frame.stage = 0;
        c->frame.gen_taken = false;
        c->frame.final_fused = false;
        c->frame.number = frame;
        c->frame.tag = next_ownv_tag(c);
        return RT_OK;
    }
    if (stage != c->frame.stage) RT_FAIL(c, RT_ERR_STATE, "rt_frame_stage: expected stage %d, got %d", c->frame.stage, stage);
    if (stage > passes + 1) RT_FAIL(c, RT_ERR_ARG, "bad stage %d", stage);
    if (stage >= 1 && stage <= passes) roles_pass(c->frame, stage - 1); /* a pure function of the stage index: a repeated _begin is harmless */
    return RT_OK;
}

static int stage_run_ranges(rt_ctx* c, Launch L, int frame, int stage, int part, int row0, int row1, int rowb0, int rowb1);
int rt_frame_stage_run_part(rt_ctx* c, int frame, int stage, int part, int row0, int row1)
{
    RT_CHECK_CTX(c);
    return stage_run_ranges(c, whole_launch(c), frame, stage, part, row0, row1, 0, 0);
}
/* the stage's second lane: the second stream, ordered behind rt_frame_stage_begin / _fork at its first use; the per-kernel
 * events belong to the main lane */
static int second_lane(rt_ctx* c, Launch& lane)
{
    if (!c->aux_used) RT_HIP(c, hipStreamWaitEvent(c->aux_stream, c->ev_stage, 0));
    c->aux_used = true;
    lane = whole_launch(c);
    lane.stream = c->aux_stream;
    lane.timed = false;
    return RT_OK;
}
/* the stage's kernels over up to two disjoint row ranges in ONE launch each (a strip's two boundary bands);
 * ranges: n x {row0, row1}, n = 1 or 2; lane 1 = the second stream (as rt_frame_stage_run_async) */
int rt_frame_stage_run_ranges(rt_ctx* c, int frame, int stage, int part, int n, const int* ranges, int lane)
{
    RT_CHECK_CTX(c);
    if (!ranges || n < 1 || n > 2) RT_FAIL(c, RT_ERR_ARG, "1 or 2 row ranges");
    if (n == 2 && !(ranges[1] <= ranges[2] || ranges[3] <= ranges[0])) RT_FAIL(c, RT_ERR_ARG, "row ranges overlap");
    Launch run = whole_launch(c);
    if (lane) { const int rc = second_lane(c, run); if (rc != RT_OK) return rc; }
    return stage_run_ranges(c, run, frame, stage, part, ranges[0], ranges[1], n == 2 ? ranges[2] : 0, n == 2 ? ranges[3] : 0);
}
/* L: the lane (the stream the stage's kernels go to, whether its per-kernel events are recorded); its rows and tag are set here */
static int stage_run_ranges(rt_ctx* c, Launch L, int frame, int stage, int part, int row0, int row1, int rowb0, int rowb1)
{
    NEED_SCENE(c);
    if (stage != c->frame.stage) RT_FAIL(c, RT_ERR_STATE, "rt_frame_stage_run: expected stage %d, got %d", c->frame.stage, stage);
    if (row0 < c->row_begin) row0 = c->row_begin;
    if (row1 > c->row_end) row1 = c->row_end;
    if (rowb0 < c->row_begin) rowb0 = c->row_begin;
    if (rowb1 > c->row_end) rowb1 = c->row_end;
    if (rowb0 >= rowb1) rowb0 = rowb1 = 0;
    if (row0 >= row1) { row0 = rowb0; row1 = rowb1; rowb0 = rowb1 = 0; }
    if (row0 >= row1) return RT_OK;
    L.row0 = row0; L.row1 = row1; L.rowb0 = rowb0; L.rowb1 = rowb1;
    L.tag = c->frame.tag; /* launches of the staged frame write / trust own-visibility flags under the frame's tag */
    const int passes = c->opt.spatial_resampling_passes;
    const bool whole = covers_owned_rows(c, L);
    const bool T = L.timed && whole;
    auto mark = [&](int i) { if (T && i <= 8) hipEventRecord(c->ev[i], L.stream); };
    int rc = RT_OK;
    if (stage == 0)
    {
        mark(0);
        if (part != 2 && c->frame.clear) rc = clear_rows(c, L);
        mark(1);
        Stage0 got;
        const bool may_defer = part == 0 && whole && use_fused_stage0(c);
        if (part != 2 && rc == RT_OK) rc = raycast_or_take(c, L, frame, may_defer, got);
        /* a reuse frame answers what a tracing frame would under the same tuning: its stage 0 on this stream is the candidates' launch
         * either way, and the bracket where the raycast launch would be is empty either way */
        if (part != 2) c->frame.one_launch = got.deferred || (got.reused && !c->frame.gen_taken && may_defer);
        if (part != 2 && rc == RT_OK && whole && !got.deferred) rc = refresh_shaded_bits(c, L);
        mark(2);
        if (part != 1 && rc == RT_OK && !c->frame.gen_taken)
        {
            rc = join_tail_for(c, L, c->frame.Y); /* this frame's candidates may go where the previous frame's resolve still reads */
            if (rc == RT_OK) rc = launch_generate(c, L, frame, c->frame.Y, c->frame.X, c->opt.use_temporal_resampling != 0, got.deferred ? L.vis : nullptr, true);
        }
        if (got.deferred && rc == RT_OK) rc = refresh_shaded_bits(c, L);
        mark(3);
    }
    else if (stage <= passes)
    {
        const int k = stage - 1;
        rc = join_tail_for(c, L, c->frame.out); /* the pass's output buffer can be the one the previous frame's resolve reads */
        if (rc == RT_OK && k == passes - 1 && use_fused_final(c))
        {
            rc = join_tail(c, L); /* the kernel writes the accumulation buffer and the pixels the previous frame's tail writes */
            if (rc == RT_OK) rc = launch_spatial(c, L, frame, k, c->frame.in, c->frame.out, true);
        }
        else if (rc == RT_OK) rc = launch_spatial(c, L, frame, k, c->frame.in, c->frame.out);
        if (k < 3) mark(4 + k);
    }
    else
    {
        for (int k = passes; k < 3; ++k) mark(4 + k);
        /* rt_indirect: the resolve stage runs the pass, once, over all owned rows (the pass's counters are the context's, not a lane's) */
        if (c->indirect > 0 && !whole)
            RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_indirect: the resolve stage must run over all owned rows in one range while the toggle is on");
        /* passes == 0: the reference resolves reservoir_buffer1, which no kernel of that frame wrote
         * (10_restir_di.cpp:324-368): zeros after start-up, else what an earlier frame's last odd pass
         * left there. Logical RT_RES_1 (physical Z) holds exactly that content here, frame by frame
         * (rt_frame_stage_end keeps the logical names on the reference's buffers), so the result is the
         * reference's, stale data included. */
        const int final_phys = roles_final_phys(c->frame, passes);
        if (c->frame.final_fused)
        {
            /* the last pass has shaded (and, key 20, tone-mapped) these rows already */
            mark(7);
            if (!c->tune_fuse_tonemap) rc = launch_tone_mapping(c, L);
            mark(8);
            return rc;
        }
        const bool tail = whole && use_tail(c, L.timed); /* never while timed: mark() records on L.stream */
        Launch R = L;
        if (tail)
        {
            /* resolve + tone_mapping on the tail stream, behind everything enqueued so far (and behind the previous
             * frame's tail: same stream); the main stream does not wait for them */
            RT_HIP(c, hipEventRecord(c->tail.ev_go, L.stream));
            RT_HIP(c, hipStreamWaitEvent(c->tail.stream, c->tail.ev_go, 0));
            R.stream = c->tail.stream;
        }
        else rc = join_tail(c, L);
        /* tone_mapping reads the pixel's own accumulation value only (common/kernels/common.cu:30-74): k_resolve maps what it
         * has just written (r05; not the persistent-wavefront A/B form, which has no such parameter) */
        const bool fuse_tm = c->tune_fuse_tonemap != 0 && !c->tune_stream && c->indirect == 0;
        if (rc == RT_OK) rc = launch_resolve(c, R, final_phys, fuse_tm ? (uint32_t*)c->d_pixels : nullptr);
        mark(7);
        /* rt_indirect: the pass on the resolve's stream, over R's G-buffer set (the look-ahead stage 0 of the next frame may be writing
         * the other one); tone mapping then maps the sum in a launch of its own. Inside rt_timing's ms[7] */
        if (rc == RT_OK && c->indirect > 0) rc = launch_indirect(c, R, frame, c->indirect);
        if (rc == RT_OK && !fuse_tm) rc = launch_tone_mapping(c, R);
        mark(8);
        if (tail && rc == RT_OK)
        {
            RT_HIP(c, hipEventRecord(c->tail.ev, c->tail.stream));
            c->tail.pending_main = true;
            c->tail.phys = final_phys;
        }
        c->tail.resolve_on = tail;
    }
    return rc;
}

/* The same rows on the context's second stream: they run beside whatever the main stream is doing
 * for this stage (a strip computes its boundary rows first, posts their halo exchange, and lets the
 * interior rows fill the rest of the GPU meanwhile).
 * The lane starts after everything that was enqueued on the main stream when rt_frame_stage_begin
 * or, later, rt_frame_stage_fork was called (fork after a part the lane depends on, e.g. the
 * raycast part of stage 0), and rt_frame_stage_end joins it back into the main stream. Rows of the
 * two lanes must not overlap, and the lane must not read halo rows still in flight. */
int rt_frame_stage_fork(rt_ctx* c)
{
    RT_CHECK_CTX(c);
    if (c->aux_used) RT_FAIL(c, RT_ERR_STATE, "rt_frame_stage_fork after the stage's second lane has started");
    RT_HIP(c, hipEventRecord(c->ev_stage, c->stream));
    return RT_OK;
}
int rt_frame_stage_run_async(rt_ctx* c, int frame, int stage, int part, int row0, int row1)
{
    RT_CHECK_CTX(c);
    Launch lane;
    const int rc = second_lane(c, lane);
    return rc != RT_OK ? rc : stage_run_ranges(c, lane, frame, stage, part, row0, row1, 0, 0);
}

/* all parts of the stage (part 0); stage 0 can be split: part 1 = [clear,] raycast, part 2 = generate */
int rt_frame_stage_run(rt_ctx* c, int frame, int stage, int row0, int row1)
{
    return rt_frame_stage_run_part(c, frame, stage, 0, row0, row1);
}

int rt_frame_stage_end(rt_ctx* c, int stage)
{
    RT_CHECK_CTX(c);
    if (stage != c->frame.stage) RT_FAIL(c, RT_ERR_STATE, "rt_frame_stage_end: expected stage %d, got %d", c->frame.stage, stage);
    if (c->aux_used)
    {
        RT_HIP(c, hipEventRecord(c->ev_aux, c->aux_stream));
        RT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_aux, 0));
        c->aux_used = false;
    }
    const int passes = c->opt.spatial_resampling_passes;
    c->fuse = HaloFuse{};
    if (stage == 0) { const int rc = launch_next_raycast(c, c->frame.number); if (rc != RT_OK) return rc; }
    if (stage <= passes) { c->frame.stage = stage + 1; return RT_OK; }
    {
        /* behind this frame's resolve (all its parts: the second lane has been joined above), on the stream it ran on: the
         * look-ahead stage 0 waits for the one before the latest */
        std::swap(c->tail.ev_resolved[0], c->tail.ev_resolved[1]);
        RT_HIP(c, hipEventRecord(c->tail.ev_resolved[0], c->tail.resolve_on ? c->tail.stream : c->stream));
        if (c->tail.n_resolved < 2) ++c->tail.n_resolved;
        c->tail.resolve_on = false;
    }
    const int X = c->frame.X, Y = c->frame.Y;
    if (passes < 2)
    {
        /* logical RT_RES_0 still equals the post-temporal reservoirs: materialise the copy the
         * reference's save_temporal_reservoir makes (10_restir_di.cpp:314-321) */
        const size_t n = local_pixels(c);
        { const int jr = join_tail_for(c, whole_launch(c), X); if (jr != RT_OK) return jr; }
        c->res_tag[X] = c->res_tag[Y];
        RT_HIP(c, hipMemcpyAsync(c->d_rec[X], c->d_rec[Y], n * 64, hipMemcpyDeviceToDevice, c->stream));
        RT_HIP(c, hipMemcpyAsync(c->d_rad[X], c->d_rad[Y], n * 16, hipMemcpyDeviceToDevice, c->stream));
    }
    roles_end(c->frame, passes);
    c->frame.stage = 0;
    c->last_valid = c->timing;
    return RT_OK;
}

/* one stage of the frame (the sequence of stages: see rt_frame_stage_begin); rt_frame runs them back to back */
int rt_frame_stage(rt_ctx* c, int frame, int stage, int clear_first)
{
    RT_CHECK_CTX(c);
    int rc = rt_frame_stage_begin(c, frame, stage, clear_first);
    if (rc == RT_OK) rc = rt_frame_stage_run(c, frame, stage, c->row_begin, c->row_end);
    if (rc == RT_OK) rc = rt_frame_stage_end(c, stage);
    return rc;
}

/* physical buffer that spatial pass `stage-1` of the running frame will read (for rt_halo_*_phys) */
int rt_frame_stage_input(rt_ctx* c, int stage, int* phys)
{
    RT_CHECK_CTX(c);
    if (!phys || stage < 1 || stage != c->frame.stage) RT_FAIL(c, RT_ERR_STATE, "no such pending stage %d", stage);
    const int k = stage - 1;
    *phys = (k == 0) ? c->frame.in : c->frame.out;
    return RT_OK;
}
/* physical buffer the CURRENT stage (after its _begin) writes: stage 0 -> the candidates(+temporal)
 * buffer, spatial stage -> its output; this is what the next spatial pass will gather from */
int rt_frame_stage_output(rt_ctx* c, int stage, int* phys)
{
    RT_CHECK_CTX(c);
    if (!phys || stage != c->frame.stage) RT_FAIL(c, RT_ERR_STATE, "stage %d is not running", stage);
    *phys = (stage == 0) ? c->frame.Y : c->frame.out;
    return RT_OK;
}

int rt_frame(rt_ctx* c, int frame, int clear_first, int* final_res)
{
    RT_CHECK_CTX(c);
    NEED_SCENE(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_STATE, "rt_frame is for single-strip contexts; strips run rt_frame_stage and exchange halos");
    const int passes = c->opt.spatial_resampling_passes;
    for (int st = 0; st <= passes + 1; ++st)
    {
        const int rc = rt_frame_stage(c, frame, st, clear_first);
        if (rc != RT_OK) return rc;
    }
    if (final_res) *final_res = c->frame.final_res;
    return RT_OK;
}

int rt_timing(rt_ctx* c, float ms[9])
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->last_valid) RT_FAIL(c, RT_ERR_STATE, "no timed frame (rt_timing_enable + rt_frame first)");
    RT_HIP(c, hipEventSynchronize(c->ev[8]));
    for (int k = 0; k < 8; ++k) RT_HIP(c, hipEventElapsedTime(&ms[k], c->ev[k], c->ev[k + 1]));
    RT_HIP(c, hipEventElapsedTime(&ms[8], c->ev[0], c->ev[8]));
    /* the frame's primary rays were traced beside the previous frame (rt_tuning key 14): the duration of that launch,
     * which ran concurrently with other kernels and is not part of ms[8] */
    if (c->ahead.timed_set >= 0)
    {
        RT_HIP(c, hipEventSynchronize(c->ahead.ev_t[c->ahead.timed_set][1]));
        RT_HIP(c, hipEventElapsedTime(&ms[1], c->ahead.ev_t[c->ahead.timed_set][0], c->ahead.ev_t[c->ahead.timed_set][1]));
    }
    return RT_OK;
}

int rt_stage0_one_launch(rt_ctx* c, int* one_launch)
{
    RT_CHECK_CTX(c);
    if (!one_launch) return RT_ERR_ARG;
    *one_launch = c->frame.one_launch ? 1 : 0;
    return RT_OK;
}

/* r13. A switch of its own and not an rt_tuning key: tests/golden/tuning_matrix.json pins keys 29 and 30 as unknown, and TUNING has
 * one row per key, in order. */
int rt_gbuffer_reuse(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (on && !whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_gbuffer_reuse: strip contexts trace their primary rays every frame");
    c->gbuf.reuse = on != 0;
    /* a look-ahead enqueued under the other setting is not taken: the next frame runs its own stage 0 */
    drop_look_ahead(c);
    return RT_OK;
}
/* The spatial passes with the 1/Z normalisation (k_spatial_unbiased). Changes results, so not an rt_tuning key either; counts as an option
 * change (rt_state_epoch). Touches no buffer: history written under the other setting stays and fades with the M cap. */
int rt_spatial_unbiased(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_spatial_unbiased: strip contexts hold no traced G-buffer in their halo rows");
    c->spatial_unbiased = on != 0;
    ++c->epoch;
    return RT_OK;
}
int rt_spatial_unbiased_get(rt_ctx* c, int* on)
{
    RT_CHECK_CTX(c);
    if (!on) return RT_ERR_ARG;
    *on = c->spatial_unbiased ? 1 : 0;
    return RT_OK;
}
/* r23. Temporal history gathered by reprojection where its buffer was written under another camera (temporal_reproject.h, DESIGN.md
 * section 13). Changes results after a camera move, so not an rt_tuning key; counts as an option change (rt_state_epoch) and drops the
 * look-ahead. Touches no buffer. A previous pixel can lie in another strip: whole-frame contexts only. */
int rt_temporal_reprojection(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_reprojection: a strip context holds only its own rows of the history");
    c->reproject = on != 0;
    drop_look_ahead(c);
    ++c->epoch;
    return RT_OK;
}
int rt_temporal_reprojection_get(rt_ctx* c, int* on)
{
    RT_CHECK_CTX(c);
    if (!on) return RT_ERR_ARG;
    *on = c->reproject ? 1 : 0;
    return RT_OK;
}
int rt_reservoir_camera(rt_ctx* c, int res, rt_raygen* out, int* has)
{
    RT_CHECK_CTX(c);
    NEED_RES(c, res);
    if (!out && !has) return RT_ERR_ARG;
    const HistoryTag& t = c->res_tag[c->frame.res_map[res]];
    if (has) *has = t.has ? 1 : 0;
    if (out) { if (t.has) *out = t.rg; else memset(out, 0, sizeof(*out)); }
    return RT_OK;
}
int rt_temporal_reprojection_stats(rt_ctx* c, uint64_t out[3])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk + 4 * WALK_REPROJECT, 3 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}
/* r24. Temporal history that follows triangles moved by rt_scene_update (temporal_motion.h), in effect only while
 * rt_temporal_reprojection is on. Changes results, so not an rt_tuning key; counts as an option change and drops the look-ahead. Touches
 * no reservoir buffer. On: d_tv_prev is allocated as a copy of the current vertices (no update is followed backwards); off: freed. */
int rt_temporal_motion(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_motion: a strip context holds only its own rows of the history");
    if (on && c->temporal_unbiased)
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_motion: rt_temporal_unbiased is on, and its ray from the history's origin would start in geometry that no longer exists");
    RT_HIP(c, hipSetDevice(c->device));
    drop_look_ahead(c);
    ++c->epoch;
    return kept_vertices_toggled(c, c->moved.toggle(FOLLOW_RESTIR, on != 0, scene_has_vertices(c)));
}
int rt_temporal_motion_get(rt_ctx* c, int* on)
{
    RT_CHECK_CTX(c);
    if (!on) return RT_ERR_ARG;
    *on = c->moved.on[FOLLOW_RESTIR] ? 1 : 0;
    return RT_OK;
}
int rt_reservoir_scene(rt_ctx* c, int res, uint64_t* generation, float eye[3], int* has)
{
    RT_CHECK_CTX(c);
    NEED_RES(c, res);
    if (!generation && !eye && !has) return RT_ERR_ARG;
    const HistoryTag& t = c->res_tag[c->frame.res_map[res]];
    if (has) *has = t.has ? 1 : 0;
    if (generation) *generation = t.has ? t.gen : 0;
    if (eye) for (int k = 0; k < 3; ++k) eye[k] = t.has ? t.eye[k] : 0.0f;
    return RT_OK;
}
int rt_temporal_motion_range(rt_ctx* c, uint32_t* lo, uint32_t* hi, uint64_t* generation)
{
    RT_CHECK_CTX(c);
    if (!lo && !hi && !generation) return RT_ERR_ARG;
    if (lo) *lo = c->moved.lo;
    if (hi) *hi = c->moved.hi;
    if (generation) *generation = c->moved.kept_gen;
    return RT_OK;
}
int rt_temporal_motion_stats(rt_ctx* c, uint64_t out[3])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk + 4 * WALK_MOTION, 3 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}
/* r32. History samples that follow emitters moved by rt_scene_update (light_follow.h). Changes results, so not an
 * rt_tuning key; counts as an option change and drops the look-ahead. Touches no reservoir buffer: the work happens in rt_scene_update. */
int rt_temporal_light_motion(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_light_motion: strip contexts are not re-based");
    RT_HIP(c, hipSetDevice(c->device));
    if (on && !c->d_lf_words) RT_HIP(c, hipMalloc(&c->d_lf_words, LF_COUNTER_WORDS * 8 + 32));
    if (on && !c->light_follow)
    {
        /* totals since the toggle went on */
        RT_HIP(c, hipMemsetAsync(c->d_lf_words, 0, LF_COUNTER_WORDS * 8 + 32, c->stream));
        c->lf_stats0 = 0;
    }
    c->light_follow = on != 0;
    drop_look_ahead(c);
    ++c->epoch;
    return RT_OK;
}
int rt_temporal_light_motion_get(rt_ctx* c, int* on, int* last_update_rebased)
{
    RT_CHECK_CTX(c);
    if (!on && !last_update_rebased) return RT_ERR_ARG;
    if (on) *on = c->light_follow ? 1 : 0;
    if (last_update_rebased) *last_update_rebased = c->lf_last;
    return RT_OK;
}
int rt_temporal_light_motion_stats(rt_ctx* c, uint64_t out[5])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_lf_words) RT_FAIL(c, RT_ERR_STATE, "rt_temporal_light_motion first");
    const int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    unsigned long long slots[LF_COUNTER_WORDS];
    RT_HIP(c, hipMemcpy(slots, c->d_lf_words, sizeof(slots), hipMemcpyDeviceToHost));
    out[0] = c->lf_stats0;
    for (int k = 0; k < 4; ++k)
    {
        out[1 + k] = 0;
        for (int s = 0; s < LF_COUNTER_SLOTS; ++s) out[1 + k] += slots[4 * s + k];
    }
    return RT_OK;
}
int rt_temporal_light_motion_timing(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    if (!c->lf_timed) RT_FAIL(c, RT_ERR_STATE, "rt_temporal_light_motion_timing: the last rt_scene_update did not run with the toggle and rt_timing_enable on");
    *ms = 0.0f;
    if (c->lf_launched) RT_HIP(c, hipEventElapsedTime(ms, c->lf_ev[0], c->lf_ev[1])); /* rt_scene_update synchronised behind them */
    return RT_OK;
}
int rt_temporal_light_motion_path(rt_ctx* c, int direct_max)
{
    RT_CHECK_CTX(c);
    c->lf_direct_max = direct_max < 0 ? LF_DIRECT_MAX_DEFAULT : direct_max;
    return RT_OK;
}
/* r31. The temporal merge with the 1/Z normalisation wherever its history is gathered by reprojection (temporal_unbiased.h, DESIGN.md
 * section 20), in effect only while rt_temporal_reprojection is on. Changes results, so not an rt_tuning key; counts as an option change
 * and drops the look-ahead. Touches no buffer: a history written with the toggle off may carry a travelled origin into the first
 * unbiased merge, and fades with the M cap. */
int rt_temporal_unbiased(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    if (!whole_frame(c))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_unbiased: a strip context holds only its own rows of the history");
    if (on && c->moved.on[FOLLOW_RESTIR])
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_unbiased: rt_temporal_motion is on, and the ray from the history's origin would start in geometry that no longer exists");
    c->temporal_unbiased = on != 0;
    drop_look_ahead(c);
    ++c->epoch;
    return RT_OK;
}
int rt_temporal_unbiased_get(rt_ctx* c, int* on)
{
    RT_CHECK_CTX(c);
    if (!on) return RT_ERR_ARG;
    *on = c->temporal_unbiased ? 1 : 0;
    return RT_OK;
}
int rt_temporal_unbiased_stats(rt_ctx* c, uint64_t out[4])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk + 4 * WALK_TUNBIASED, 4 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}
/* How the candidates pick their light (light_alias.h). Changes results, so not an rt_tuning key; counts as an
 * option change (rt_state_epoch) and drops the look-ahead, whose stage 0 drew its candidates under the other setting. Touches no
 * buffer: a stored record carries a contribution weight, valid under either sampling. */
int rt_light_sampling(rt_ctx* c, int mode)
{
    RT_CHECK_CTX(c);
    if (mode != RT_LIGHTS_UNIFORM && mode != RT_LIGHTS_POWER) RT_FAIL(c, RT_ERR_ARG, "rt_light_sampling: unknown mode %d", mode);
    c->light_mode = mode;
    drop_look_ahead(c);
    ++c->epoch;
    return RT_OK;
}
int rt_light_sampling_get(rt_ctx* c, int* mode)
{
    RT_CHECK_CTX(c);
    if (!mode) return RT_ERR_ARG;
    *mode = c->light_mode;
    return RT_OK;
}
int rt_light_table(rt_ctx* c, uint32_t* thr, uint32_t* alias, uint64_t* K, uint32_t n)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "rt_light_table before rt_scene_set");
    if (n != (uint32_t)c->n_lights) RT_FAIL(c, RT_ERR_ARG, "rt_light_table: %u entries asked for, the scene has %d lights", n, c->n_lights);
    for (uint32_t i = 0; i < n; ++i)
    {
        if (thr) thr[i] = c->h_alias[i].thr;
        if (alias) alias[i] = c->h_alias[i].alias;
        if (K) K[i] = c->h_alias_K[i];
    }
    return RT_OK;
}
/* Distance-aware light selection (light_grid.h). Like rt_light_sampling: changes results, so not an rt_tuning
 * key; counts as an option change and drops the look-ahead; touches no reservoir buffer. With a scene present the tables are built
 * here, from the device's triangles; otherwise by rt_scene_set. */
int rt_light_grid(rt_ctx* c, int cells_per_axis, int clusters)
{
    RT_CHECK_CTX(c);
    if (cells_per_axis != 0)
    {
        if (cells_per_axis < 1 || cells_per_axis > kGridMaxCells || clusters < 1 || clusters > kGridMaxClusters)
            RT_FAIL(c, RT_ERR_ARG, "rt_light_grid: %d cells per axis (1..%d) and %d clusters (1..%d)", cells_per_axis, kGridMaxCells, clusters, kGridMaxClusters);
        if (!whole_frame(c)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_light_grid: not built for strip contexts");
    }
    else clusters = 0;
    if (cells_per_axis != c->grid_cells || clusters != c->grid_clusters)
    {
        if (c->has_scene)
        {
            /* every stream that may still read the tables, as rt_scene_set */
            RT_HIP(c, hipSetDevice(c->device));
            { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
            if (c->own_stream && c->own_stream != c->stream) RT_HIP(c, hipStreamSynchronize(c->own_stream));
            if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream));
        }
        if (cells_per_axis == 0) free_light_grid(c);
        else if (c->has_scene && c->n_tris > 0)
        {
            if (c->h_grid_tris.size() != (size_t)c->n_tris * 15)
            {
                c->h_grid_tris.resize((size_t)c->n_tris * 15);
                RT_HIP(c, hipMemcpy(c->h_grid_tris.data(), c->d_tris, (size_t)c->n_tris * 60, hipMemcpyDeviceToHost));
            }
            const int old_cells = c->grid_cells, old_clusters = c->grid_clusters;
            c->grid_cells = cells_per_axis; c->grid_clusters = clusters;
            const int rg = build_light_grid(c, c->h_lights, c->stream);
            if (rg != RT_OK)
            {
                /* nothing changes: the old tables are gone, so the old request is built again (or the grid is off) */
                c->grid_cells = old_cells; c->grid_clusters = old_clusters;
                const std::string why = c->err;
                if (old_cells == 0 || build_light_grid(c, c->h_lights, c->stream) != RT_OK) { c->grid_cells = c->grid_clusters = 0; free_light_grid(c); }
                c->err = why;
                return rg;
            }
        }
        c->grid_cells = cells_per_axis; c->grid_clusters = clusters;
    }
    drop_look_ahead(c);
    ++c->epoch;
    return RT_OK;
}
int rt_light_grid_get(rt_ctx* c, int* cells_per_axis, int* clusters, int* clusters_built)
{
    RT_CHECK_CTX(c);
    if (cells_per_axis) *cells_per_axis = c->grid_cells;
    if (clusters) *clusters = c->grid_clusters;
    if (clusters_built) *clusters_built = c->grid_built ? (int)c->h_grid.B : 0;
    return RT_OK;
}
int rt_light_grid_build_ms(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (!ms) return RT_ERR_ARG;
    *ms = c->grid_build_ms;
    return RT_OK;
}
int rt_light_grid_table(rt_ctx* c, float bounds[9], uint32_t* cluster_of, uint32_t* perm, uint32_t* run_start, uint32_t* run_thr, uint32_t* run_alias,
                        uint64_t* run_K, uint32_t* cell_thr, uint32_t* cell_alias, uint64_t* cell_K, float* cell_prob, uint32_t n_lights,
                        uint32_t n_cell_slots)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "rt_light_grid_table before rt_scene_set");
    if (c->grid_cells == 0 || !c->grid_built) RT_FAIL(c, RT_ERR_STATE, "rt_light_grid_table: the light grid is off");
    const LightGrid& g = c->h_grid;
    const size_t n = g.L ? g.cell_slots() : 0;
    if (n_lights != g.L || (size_t)n_cell_slots != n)
        RT_FAIL(c, RT_ERR_ARG, "rt_light_grid_table: %u lights and %u cell slots asked for, the grid has %u and %zu", n_lights, n_cell_slots, g.L, n);
    if (bounds)
        for (int a = 0; a < 3; ++a) { bounds[a] = g.lo[a]; bounds[3 + a] = g.hi[a]; bounds[6 + a] = g.inv[a]; }
    if (perm) memcpy(perm, g.perm.data(), (size_t)g.L * 4);
    for (uint32_t p = 0; p < g.L && run_K; ++p) run_K[p] = g.run_K[p];
    for (size_t k = 0; k < n && cell_K; ++k) cell_K[k] = g.cell_K[k];
    if (g.L == 0) { if (run_start) run_start[0] = 0u; return RT_OK; }
    /* everything the device holds comes back from the device */
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    if (cluster_of) RT_HIP(c, hipMemcpy(cluster_of, c->d_grid_cluster_of, (size_t)g.L * 4, hipMemcpyDeviceToHost));
    if (run_start)
    {
        std::vector<GridRun> runs(g.B);
        RT_HIP(c, hipMemcpy(runs.data(), c->d_grid_runs, (size_t)g.B * sizeof(GridRun), hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < g.B; ++r) run_start[r] = runs[r].start;
        run_start[g.B] = runs[g.B - 1].start + runs[g.B - 1].n;
    }
    if (run_thr || run_alias)
    {
        std::vector<AliasSlot> t(g.L);
        RT_HIP(c, hipMemcpy(t.data(), c->d_grid_run_slots, (size_t)g.L * sizeof(AliasSlot), hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p < g.L; ++p) { if (run_thr) run_thr[p] = t[p].thr; if (run_alias) run_alias[p] = t[p].alias; }
    }
    if (cell_thr || cell_alias)
    {
        std::vector<AliasSlot> t(n);
        RT_HIP(c, hipMemcpy(t.data(), c->d_grid_cells, n * sizeof(AliasSlot), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; ++k) { if (cell_thr) cell_thr[k] = t[k].thr; if (cell_alias) cell_alias[k] = t[k].alias; }
    }
    if (cell_prob) RT_HIP(c, hipMemcpy(cell_prob, c->d_grid_cell_prob, n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}
int rt_primary_launches(rt_ctx* c, uint64_t* n)
{
    RT_CHECK_CTX(c);
    if (!n) return RT_ERR_ARG;
    *n = c->gbuf.primary_launches;
    return RT_OK;
}

int rt_local_rows(rt_ctx* c, int* first_row, int* n_rows)
{
    RT_CHECK_CTX(c);
    if (first_row) *first_row = c->lrow0;
    if (n_rows) *n_rows = c->lrows;
    return RT_OK;
}

int rt_download(rt_ctx* c, int buf, void* dst, size_t bytes)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    if (!dst) RT_FAIL(c, RT_ERR_ARG, "null dst");
    const size_t n = local_pixels(c);
    switch (buf)
    {
        case RT_BUF_VISIBILITY:
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            RT_HIP(c, hipMemcpyAsync(dst, c->gbuf.vis, bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        case RT_BUF_ACCUMULATION:
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            RT_HIP(c, hipMemcpyAsync(dst, c->d_accum, bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        case RT_BUF_PIXELS:
            if (bytes != n * 4) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 4);
            RT_HIP(c, hipMemcpyAsync(dst, c->d_pixels, bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        case RT_BUF_DENOISED:
        case RT_BUF_DENOISE_GUIDE:
            if (!c->dn_valid) RT_FAIL(c, RT_ERR_STATE, "buffer %d is written by rt_denoise, which has not run on this context", buf);
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            RT_HIP(c, hipMemcpyAsync(dst, buf == RT_BUF_DENOISED ? c->d_dn_hdr : c->d_dn_vis, bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        case RT_BUF_DENOISE_HISTORY:
            if (!c->dt_valid) RT_FAIL(c, RT_ERR_STATE, "no rt_denoise_temporal history (none since the context, the scene or the last reset)");
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            RT_HIP(c, hipMemcpyAsync(dst, c->d_dt_mom[c->dt_cur], bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        case RT_BUF_RES_0:
        case RT_BUF_RES_1:
        case RT_BUF_RES_TEMPORAL:
        {
            if (bytes != n * 76) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 76);
            const int phys = c->frame.res_map[buf - RT_BUF_RES_0];
            int rc = ensure_stage(c, n * 76);
            if (rc != RT_OK) return rc;
            k_res_to_ref<<<(int)((n + 255) / 256), 256, 0, c->stream>>>((int)n, c->d_rec[phys], c->d_rad[phys], (uint32_t*)c->d_stage);
            RT_HIP(c, hipGetLastError());
            RT_HIP(c, hipMemcpyAsync(dst, c->d_stage, bytes, hipMemcpyDeviceToHost, c->stream));
            break;
        }
        default: RT_FAIL(c, RT_ERR_ARG, "unknown buffer %d", buf);
    }
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

int rt_upload(rt_ctx* c, int buf, const void* src, size_t bytes)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    JOIN_SPEC(c);
    if (!src) RT_FAIL(c, RT_ERR_ARG, "null src");
    const size_t n = local_pixels(c);
    switch (buf)
    {
        case RT_BUF_VISIBILITY:
        {
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            NEED_SCENE(c);
            RT_HIP(c, hipMemcpyAsync(c->gbuf.vis, src, bytes, hipMemcpyHostToDevice, c->stream));
            FrameParams P = make_params(c, whole_launch(c), 0, 0);
            P.row0 = c->lrow0; P.row1 = c->lrow0 + c->lrows; /* all rows held, halos included */
            k_gbuffer_from_vis<<<tile_grid(c->W, c->lrows), BLOCK, 0, c->stream>>>(make_scene(c), P, c->gbuf.vis, c->gbuf.g0, c->gbuf.g1);
            RT_HIP(c, hipGetLastError());
            gbuffer_written(c, whole_launch(c), GBUF_UPLOADED);
            ++c->epoch;
            break;
        }
        case RT_BUF_ACCUMULATION:
            if (bytes != n * 16) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 16);
            RT_HIP(c, hipMemcpyAsync(c->d_accum, src, bytes, hipMemcpyHostToDevice, c->stream));
            break;
        case RT_BUF_RES_0:
        case RT_BUF_RES_1:
        case RT_BUF_RES_TEMPORAL:
        {
            if (bytes != n * 76) RT_FAIL(c, RT_ERR_ARG, "size mismatch: want %zu", n * 76);
            if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "upload RT_BUF_VISIBILITY (or rt_raycast) before reservoirs");
            ++c->res_epoch;
            const int phys = c->frame.res_map[buf - RT_BUF_RES_0];
            tag_reservoir(c, phys); /* its shaded bits come from the current G-buffer: the current camera's pixels */
            /* the record keeps M in 30 bits: refuse what it cannot hold rather than truncate */
            for (size_t i = 0; i < n; ++i)
            {
                const int32_t M = ((const rt_reservoir*)src)[i].M;
                if (M < 0 || M >= (1 << 30)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "reservoir %zu has M = %d outside [0, 2^30)", i, M);
            }
            int rc = ensure_stage(c, n * 76);
            if (rc != RT_OK) return rc;
            RT_HIP(c, hipMemcpyAsync(c->d_stage, src, bytes, hipMemcpyHostToDevice, c->stream));
            k_res_from_ref<<<(int)((n + 255) / 256), 256, 0, c->stream>>>((int)n, (const uint32_t*)c->d_stage, c->gbuf.g1, c->d_rec[phys], c->d_rad[phys]);
            RT_HIP(c, hipGetLastError());
            break;
        }
        default: RT_FAIL(c, RT_ERR_ARG, "buffer %d cannot be uploaded", buf);
    }
    RT_HIP(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

size_t rt_halo_bytes(rt_ctx* c, int n_rows) { return c ? (size_t)n_rows * (size_t)c->W * 80 : 0; }

static int halo_range(rt_ctx* c, int row0, int n_rows)
{
    if (n_rows <= 0 || row0 < c->lrow0 || row0 + n_rows > c->lrow0 + c->lrows)
        RT_FAIL(c, RT_ERR_ARG, "rows [%d,%d) outside the rows held [%d,%d)", row0, row0 + n_rows, c->lrow0, c->lrow0 + c->lrows);
    return RT_OK;
}
/* res: RT_RES_* (logical) or RT_RES_PHYS + p for the physical buffer p that
 * rt_frame_stage_input reported */
static int halo_phys(rt_ctx* c, int res)
{
    if (res >= RT_RES_PHYS && res < RT_RES_PHYS + 5 && c->d_rec[res - RT_RES_PHYS]) return res - RT_RES_PHYS;
    if (res >= 0 && res <= 2) return c->frame.res_map[res];
    return -1;
}
int rt_halo_pack(rt_ctx* c, int res, int row0, int n_rows, void* device_dst)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    const int phys = halo_phys(c, res);
    if (phys < 0) RT_FAIL(c, RT_ERR_ARG, "bad reservoir buffer id %d", res);
    int rc = halo_range(c, row0, n_rows);
    if (rc != RT_OK) return rc;
    const size_t off = (size_t)(row0 - c->lrow0) * c->W, n = (size_t)n_rows * c->W;
    RT_HIP(c, hipMemcpyAsync(device_dst, c->d_rec[phys] + 4 * off, n * 64, hipMemcpyDeviceToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync((char*)device_dst + n * 64, c->d_rad[phys] + off, n * 16, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}
int rt_halo_unpack(rt_ctx* c, int res, int row0, int n_rows, const void* device_src)
{
    RT_CHECK_CTX(c);
    JOIN_TAIL(c);
    const int phys = halo_phys(c, res);
    if (phys < 0) RT_FAIL(c, RT_ERR_ARG, "bad reservoir buffer id %d", res);
    int rc = halo_range(c, row0, n_rows);
    if (rc != RT_OK) return rc;
    const size_t off = (size_t)(row0 - c->lrow0) * c->W, n = (size_t)n_rows * c->W;
    RT_HIP(c, hipMemcpyAsync(c->d_rec[phys] + 4 * off, device_src, n * 64, hipMemcpyDeviceToDevice, c->stream));
    RT_HIP(c, hipMemcpyAsync(c->d_rad[phys] + off, (const char*)device_src + n * 64, n * 16, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}

/* ---- sparse halos: see k_halo_mark. side 0 = the strip below (rows [row_begin-halo, row_begin)),
 * side 1 = the strip above (rows [row_end, row_end+halo)). ---- */
static int halo_side_region(rt_ctx* c, int side, int* r0, int* n)
{
    if (side == 0) { *r0 = c->lrow0; *n = c->row_begin - c->lrow0; }
    else if (side == 1) { *r0 = c->row_end; *n = c->lrow0 + c->lrows - c->row_end; }
    else RT_FAIL(c, RT_ERR_ARG, "side must be 0 or 1");
    if (*n <= 0) RT_FAIL(c, RT_ERR_STATE, "no halo rows on side %d", side);
    return RT_OK;
}
size_t rt_halo_bitmap_words(rt_ctx* c, int n_rows)
{
    if (!c) return 0;
    const size_t nw = ((size_t)n_rows * c->W + 31) / 32;
    return 1 + 2 * nw; /* count, bits, prefix; only the first 1 + nw words travel */
}
size_t rt_halo_flags_bytes(rt_ctx* c, int n_rows) { return c ? (size_t)n_rows * c->W : 0; }
int rt_halo_flags_pack(rt_ctx* c, int row0, int n_rows, void* device_dst)
{
    RT_CHECK_CTX(c);
    int rc = halo_range(c, row0, n_rows);
    if (rc != RT_OK) return rc;
    const int n = n_rows * c->W;
    k_halo_flags<true><<<(n + 255) / 256, 256, 0, c->stream>>>(c->gbuf.g1, (size_t)(row0 - c->lrow0) * c->W, n, (uint8_t*)device_dst);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_halo_flags_unpack(rt_ctx* c, int row0, int n_rows, const void* device_src)
{
    RT_CHECK_CTX(c);
    int rc = halo_range(c, row0, n_rows);
    if (rc != RT_OK) return rc;
    if (row0 < c->row_end && row0 + n_rows > c->row_begin) RT_FAIL(c, RT_ERR_ARG, "flags may only be unpacked into halo rows");
    const int n = n_rows * c->W;
    for (int set = 0; set < rt_ctx::NGSET; ++set)
        if (c->gbuf.set[set][2])
            k_halo_flags<false><<<(n + 255) / 256, 256, 0, c->stream>>>(c->gbuf.set[set][2], (size_t)(row0 - c->lrow0) * c->W, n, (uint8_t*)const_cast<void*>(device_src));
    RT_HIP(c, hipGetLastError());
    c->gbuf.shaded_bits_stale = true; /* the LDS-staged spatial pass reads these rows' bits too */
    c->mark_bits_epoch = 0;      /* and the halo marks' cached rows */
    if (row0 == c->lrow0 && row0 + n_rows == c->row_begin) c->halo_flags_epoch[0] = c->epoch;
    if (row0 == c->row_end && row0 + n_rows == c->lrow0 + c->lrows) c->halo_flags_epoch[1] = c->epoch;
    return RT_OK;
}
/* records of the neighbour on `side` that spatial passes [pass, pass + n_pass) of `frame` will
 * gather: n_pass consecutive bitmaps of rt_halo_bitmap_words() words each, one launch */
int rt_halo_mark_sides(rt_ctx* c, int frame, int pass, int n_pass, void* bitmaps_side0, void* bitmaps_side1)
{
    RT_CHECK_CTX(c);
    if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "no G-buffer yet");
    if (n_pass <= 0 || (!bitmaps_side0 && !bitmaps_side1)) return RT_OK;
    HaloRegions R = {};
    R.quick = c->tune_mark_quick;
    void* bm[2] = {bitmaps_side0, bitmaps_side1};
    for (int side = 0; side < 2; ++side)
    {
        if (!bm[side]) continue;
        int rc = halo_side_region(c, side, &R.row0[side], &R.rows[side]);
        if (rc != RT_OK) return rc;
        if (c->halo_flags_epoch[side] != c->epoch)
            RT_FAIL(c, RT_ERR_STATE, "rt_halo_mark: the neighbour's shaded flags (rt_halo_flags_unpack of all %d halo rows on side %d) "
                                     "must be refreshed after a camera, scene or option change", R.rows[side], side);
        R.words[side] = rt_halo_bitmap_words(c, R.rows[side]);
        R.bitmaps[side] = (uint32_t*)bm[side];
    }
    /* both sides in ONE allocation, side 0 first (rt_mg's arena): cleared with one memset, whatever lies between included */
    const size_t bytes0 = R.words[0] * 4 * (size_t)n_pass, bytes1 = R.words[1] * 4 * (size_t)n_pass;
    const bool together = bm[0] && bm[1] && (char*)bm[1] >= (char*)bm[0] + bytes0 && (size_t)((char*)bm[1] - (char*)bm[0]) <= 2 * bytes0 + (1u << 20);
    if (together) RT_HIP(c, hipMemsetAsync(bm[0], 0, (size_t)((char*)bm[1] - (char*)bm[0]) + bytes1, c->stream));
    else
    {
        if (bm[0]) RT_HIP(c, hipMemsetAsync(bm[0], 0, bytes0, c->stream));
        if (bm[1]) RT_HIP(c, hipMemsetAsync(bm[1], 0, bytes1, c->stream));
    }
    /* only own rows within `halo` rows of a side can reach across it: one band per side, one launch over both (or
     * over all own rows when the bands meet) */
    const int lo_end = c->row_begin + c->halo < c->row_end ? c->row_begin + c->halo : c->row_end;
    const int hi_beg = c->row_end - c->halo > c->row_begin ? c->row_end - c->halo : c->row_begin;
    Launch L = whole_launch(c); /* its rows: the launch's extent */
    if (bm[0] && bm[1] && lo_end < hi_beg) { L.row1 = lo_end; L.rowb0 = hi_beg; L.rowb1 = c->row_end; }
    else if (bm[0] && !bm[1]) L.row1 = lo_end;
    else if (!bm[0]) L.row0 = hi_beg;
    const FrameParams P = make_params(c, L, frame, pass, K_OTHER);
    const int grid = launch_grid(c, L);
    /* marks collected per workgroup in an LDS window, one global atomic per non-zero word (frame_kernels.h) where it applies */
    const bool window = c->tune_mark_window && (c->W % 32) == 0 && n_pass <= MARK_MAX_PASSES && halo_rows_needed(c->opt) <= SPL_HALO;
    if (window)
    {
        /* the shaded bit of every local pixel (own rows + the neighbours' flags in the halo rows), rebuilt in front of every
         * mark on the marking stream: ~3 us, and no staleness to track across the two G-buffer sets of the pipelined stage 0 */
        const int words = c->W / 32;
        if (!c->d_mark_bits) RT_HIP(c, hipMalloc(&c->d_mark_bits, (size_t)c->lrows * words * 4));
        /* r05: the bits are a function of the camera, the scene and the options (own rows: what raycast writes, the same in both
         * G-buffer sets; halo rows: the neighbours' flags, unpacked once per epoch), not of the frame: built once per epoch
         * from a G-buffer traced under it and kept (r04 rebuilt them in front of every mark: 13 us alone, 84 us beside a 4K
         * strip's raycast). A G-buffer of another epoch (marks before the first raycast after a change) is not cached.
         * Ordering: a mark that finds the cache valid may run on another stream than the mark that built it — ev_mark_bits. */
        const bool cacheable = c->gbuf.epoch == c->epoch;
        if (!(cacheable && c->mark_bits_epoch == c->epoch) || !c->tune_mark_cache)
        {
            if (c->mark_bits_event_valid) RT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_mark_bits, 0)); /* earlier readers / writer */
            k_shaded_bitmap<<<dim3((c->W + 255) / 256, c->lrows), 256, 0, c->stream>>>(c->W, c->lrows, c->gbuf.g1, c->d_mark_bits);
            RT_HIP(c, hipGetLastError());
            c->mark_bits_epoch = cacheable ? c->epoch : 0;
            c->mark_bits_rebuilt = true;
        }
        else RT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_mark_bits, 0)); /* the build (and every mark since) is in front of this one */
        k_halo_mark<true><<<dim3(grid, c->tune_mark_split ? n_pass : 1), BLOCK, 0, c->stream>>>(P, c->gbuf.g1, c->d_mark_bits, R, pass, n_pass);
    }
    else k_halo_mark<false><<<dim3(grid, c->tune_mark_split ? n_pass : 1), BLOCK, 0, c->stream>>>(P, c->gbuf.g1, nullptr, R, pass, n_pass);
    RT_HIP(c, hipGetLastError());
    if (window)
    {
        /* whoever rebuilds the bits next (another stream, another epoch) waits for this reader; whoever reads them next waits for
         * the build in front of it */
        RT_HIP(c, hipEventRecord(c->ev_mark_bits, c->stream));
        c->mark_bits_event_valid = true;
    }
    {
        const size_t wmax = R.words[0] > R.words[1] ? R.words[0] : R.words[1];
        k_halo_scan_sides<<<dim3(halo_scan_chunks((int)((wmax - 1) / 2)), n_pass, 2), HALO_SCAN_THREADS, 0, c->stream>>>(R);
    }
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_halo_mark(rt_ctx* c, int frame, int pass, int n_pass, int side, void* device_bitmaps)
{
    RT_CHECK_CTX(c);
    if (side != 0 && side != 1) RT_FAIL(c, RT_ERR_ARG, "side must be 0 or 1");
    if (!device_bitmaps) RT_FAIL(c, RT_ERR_ARG, "null pointer");
    return rt_halo_mark_sides(c, frame, pass, n_pass, side == 0 ? device_bitmaps : nullptr, side == 1 ? device_bitmaps : nullptr);
}
/* rebuild the prefix part of `count` consecutive bitmaps received from a neighbour */
int rt_halo_scan(rt_ctx* c, int n_rows, int count, void* device_bitmaps)
{
    RT_CHECK_CTX(c);
    if (count <= 0) return RT_OK;
    const size_t words = rt_halo_bitmap_words(c, n_rows);
    k_halo_scan<<<dim3(halo_scan_chunks((int)((words - 1) / 2)), count), HALO_SCAN_THREADS, 0, c->stream>>>((uint32_t*)device_bitmaps, (int)((words - 1) / 2), words);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
static int halo_sparse(rt_ctx* c, bool pack, int res, int n, const int* row0, const int* n_rows, const void* const* device_bitmap, void* const* device_list)
{
    const int phys = halo_phys(c, res);
    if (phys < 0) RT_FAIL(c, RT_ERR_ARG, "bad reservoir buffer id %d", res);
    if (n <= 0) return RT_OK;
    if (n > 2) RT_FAIL(c, RT_ERR_ARG, "at most two row ranges per call");
    HaloLists Hh = {};
    int most = 0;
    for (int i = 0; i < n; ++i)
    {
        int rc = halo_range(c, row0[i], n_rows[i]);
        if (rc != RT_OK) return rc;
        Hh.bitmap[i] = (const uint32_t*)device_bitmap[i];
        Hh.n_pix[i] = n_rows[i] * c->W;
        Hh.nw[i] = (int)((rt_halo_bitmap_words(c, n_rows[i]) - 1) / 2);
        Hh.region_off[i] = (size_t)(row0[i] - c->lrow0) * c->W;
        Hh.list[i] = (float4*)device_list[i];
        if (Hh.n_pix[i] > most) most = Hh.n_pix[i];
    }
    const dim3 grid((most + 255) / 256, n);
    if (pack) k_halo_sparse<true><<<grid, 256, 0, c->stream>>>(Hh, c->d_rec[phys], c->d_rad[phys]);
    else k_halo_sparse<false><<<grid, 256, 0, c->stream>>>(Hh, c->d_rec[phys], c->d_rad[phys]);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
/* The running spatial stage reads its halo records from the received lists and writes the records its neighbours marked
 * to the send lists itself (no rt_halo_unpack_sparse before / rt_halo_pack_sparse after it): call between
 * rt_frame_stage_begin(stage in 1..passes) and the _run calls it shall apply to; rt_frame_stage_end clears it. Regions
 * are the context's own: received records belong to the halo rows below (side 0) / above (side 1) the strip, sent ones to
 * the first / last `halo` owned rows. Lists and bitmaps as for the separate calls. */
int rt_halo_fuse_set(rt_ctx* c, const rt_halo_fuse* f)
{
    RT_CHECK_CTX(c);
    c->fuse = HaloFuse{};
    if (!f) return RT_OK;
    if (c->frame.stage < 1 || c->frame.stage > c->opt.spatial_resampling_passes) RT_FAIL(c, RT_ERR_STATE, "rt_halo_fuse_set outside a spatial stage");
    if (use_lds_spatial(c)) RT_FAIL(c, RT_ERR_UNSUPPORTED, "the LDS-staged spatial variant reads halo rows, not lists");
    HaloFuse F = {};
    F.rows = c->halo;
    F.nw = (int)(((size_t)c->halo * c->W + 31) / 32);
    for (int side = 0; side < 2; ++side)
    {
        const bool has = side == 0 ? c->row_begin > 0 : c->row_end < c->H;
        if ((f->need_bitmap[side] || f->recv_list[side] || f->give_bitmap[side] || f->send_list[side]) && !has)
            RT_FAIL(c, RT_ERR_ARG, "no neighbour on side %d", side);
        if (!has) continue;
        int r0 = 0, n = 0;
        const int rc = halo_side_region(c, side, &r0, &n);
        if (rc != RT_OK) return rc;
        if (n != c->halo || c->row_end - c->row_begin < c->halo) RT_FAIL(c, RT_ERR_STATE, "fused halos need full %d-row regions", c->halo);
        if ((f->need_bitmap[side] != nullptr) != (f->recv_list[side] != nullptr) || (f->give_bitmap[side] != nullptr) != (f->send_list[side] != nullptr))
            RT_FAIL(c, RT_ERR_ARG, "bitmap and list go together");
        F.need_bm[side] = (const uint32_t*)f->need_bitmap[side];
        F.recv[side] = (const float4*)f->recv_list[side];
        F.need_row0[side] = r0;
        F.give_bm[side] = (const uint32_t*)f->give_bitmap[side];
        F.send[side] = (float4*)f->send_list[side];
        F.give_row0[side] = side == 0 ? c->row_begin : c->row_end - c->halo;
    }
    c->fuse = F;
    return RT_OK;
}
int rt_halo_pack_sparse(rt_ctx* c, int res, int row0, int n_rows, const void* device_bitmap, void* device_dst)
{
    RT_CHECK_CTX(c);
    return halo_sparse(c, true, res, 1, &row0, &n_rows, &device_bitmap, &device_dst);
}
int rt_halo_unpack_sparse(rt_ctx* c, int res, int row0, int n_rows, const void* device_bitmap, const void* device_src)
{
    RT_CHECK_CTX(c);
    void* src = const_cast<void*>(device_src);
    return halo_sparse(c, false, res, 1, &row0, &n_rows, &device_bitmap, &src);
}
/* the same for up to two row ranges (both neighbours) in one launch */
int rt_halo_pack_sparse_ranges(rt_ctx* c, int res, int n, const int* row0, const int* n_rows, const void* const* device_bitmaps, void* const* device_dsts)
{
    RT_CHECK_CTX(c);
    return halo_sparse(c, true, res, n, row0, n_rows, device_bitmaps, device_dsts);
}
int rt_halo_unpack_sparse_ranges(rt_ctx* c, int res, int n, const int* row0, const int* n_rows, const void* const* device_bitmaps, const void* const* device_srcs)
{
    RT_CHECK_CTX(c);
    return halo_sparse(c, false, res, n, row0, n_rows, device_bitmaps, const_cast<void* const*>(device_srcs));
}

/* ---- hooks of the native strip driver (strip_mg.cpp), plain C-ABI like everything else ---- */
int rt_state_epoch(rt_ctx* c, uint64_t* epoch)
{
    RT_CHECK_CTX(c);
    if (!epoch) return RT_ERR_ARG;
    *epoch = c->epoch;
    return RT_OK;
}
/* the context's tail stream (resolve + tone_mapping of a staged frame, rt_tuning key 17): a strip driver enqueues its halo-plan
 * marks there instead of on a stream of its own — one hardware queue less to compete for, and a plan is needed a frame later */
int rt_side_stream(rt_ctx* c, int which, void** hip_stream)
{
    RT_CHECK_CTX(c);
    if (!hip_stream || which != 0) RT_FAIL(c, RT_ERR_ARG, "which: 0 = tail stream");
    *hip_stream = (void*)c->tail.stream;
    return RT_OK;
}
/* n <= 8 device-to-device copies in one launch on the current stream */
int rt_copy_parts(rt_ctx* c, int n, const void* const* src, void* const* dst, const size_t* bytes)
{
    RT_CHECK_CTX(c);
    if (n < 0 || n > 8 || (n > 0 && (!src || !dst || !bytes))) RT_FAIL(c, RT_ERR_ARG, "0..8 parts");
    if (n == 0) return RT_OK;
    CopyParts P;
    memset(&P, 0, sizeof(P));
    size_t largest = 0;
    for (int i = 0; i < n; ++i)
    {
        if (bytes[i] && (!src[i] || !dst[i])) RT_FAIL(c, RT_ERR_ARG, "null part %d", i);
        P.src[i] = (const char*)src[i]; P.dst[i] = (char*)dst[i]; P.bytes[i] = bytes[i];
        largest = bytes[i] > largest ? bytes[i] : largest;
    }
    if (largest == 0) return RT_OK;
    const size_t want = (largest / 16 + 255) / 256;
    /* up to 2048 workgroups per part: fewer, fatter ones (8 / 32) were slower on a busy GPU, profiles/r04_strip_interior_late.txt */
    const unsigned gx = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    k_copy_parts<<<dim3(gx, (unsigned)n), 256, 0, c->stream>>>(P);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
/* WIRE_MODEL (strip_mg.cpp): phase 0 = stamp the GPU clock on the current stream (in front of an exchange), phase 1 = hold
 * the current stream until `ns` nanoseconds after that stamp (behind the exchange). slot: 0..7. A slot's stamp and wait must be
 * enqueued on ONE stream, and a slot must not be shared between streams: stream order is what keeps the next stamp of a slot behind
 * the wait that still reads it (the strip driver: slots 0-3 for exchanges on the main stream, 4-7 on the communication stream). */
int rt_wire_delay(rt_ctx* c, int phase, int slot, unsigned long long ns)
{
    RT_CHECK_CTX(c);
    if (slot < 0 || slot > 7 || (phase != 0 && phase != 1)) RT_FAIL(c, RT_ERR_ARG, "rt_wire_delay: phase 0 / 1, slot 0..7");
    /* one sleeping wavefront holds the stream for `ns`: a mistyped RT_MG_WIRE_GBS / RT_MG_WIRE_LAT_US must not park it until the
     * watchdog fires. 5 ms = a 4K frame's whole dense halo at a hundredth of an xGMI link. */
    if (ns > 5000000ull) RT_FAIL(c, RT_ERR_ARG, "rt_wire_delay: %llu ns is more than the 5 ms a modelled exchange may take (RT_MG_WIRE_GBS / RT_MG_WIRE_LAT_US?)", ns);
    if (!c->d_wire)
    {
        RT_HIP(c, hipMalloc(&c->d_wire, 8 * sizeof(unsigned long long)));
        RT_HIP(c, hipMemset(c->d_wire, 0, 8 * sizeof(unsigned long long)));
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000; /* 100 MHz */
        c->wall_khz = khz;
    }
    if (phase == 0) k_wire_stamp<<<1, 1, 0, c->stream>>>(c->d_wire + slot);
    else k_wire_wait<<<1, 64, 0, c->stream>>>(c->d_wire + slot, (unsigned long long)((double)ns * (double)c->wall_khz * 1e-6));
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}
int rt_get_stream(rt_ctx* c, void** hip_stream)
{
    RT_CHECK_CTX(c);
    if (!hip_stream) return RT_ERR_ARG;
    *hip_stream = (void*)c->stream;
    return RT_OK;
}
int rt_geometry(rt_ctx* c, int* width, int* height, int* row_begin, int* row_end, int* halo)
{
    RT_CHECK_CTX(c);
    if (width) *width = c->W;
    if (height) *height = c->H;
    if (row_begin) *row_begin = c->row_begin;
    if (row_end) *row_end = c->row_end;
    if (halo) *halo = c->halo;
    return RT_OK;
}
/* device addresses of `n_rows` storage rows of a reservoir buffer (64-B records, 16-B radiance side
 * records): dense halos are sent from and received into the buffers themselves, no staging copy */
int rt_res_region(rt_ctx* c, int res, int row0, int n_rows, void** rec, size_t* rec_bytes, void** rad, size_t* rad_bytes)
{
    RT_CHECK_CTX(c);
    const int phys = halo_phys(c, res);
    if (phys < 0) RT_FAIL(c, RT_ERR_ARG, "bad reservoir buffer id %d", res);
    int rc = halo_range(c, row0, n_rows);
    if (rc != RT_OK) return rc;
    const size_t off = (size_t)(row0 - c->lrow0) * c->W, n = (size_t)n_rows * c->W;
    if (rec) *rec = (void*)(c->d_rec[phys] + 4 * off);
    if (rec_bytes) *rec_bytes = n * 64;
    if (rad) *rad = (void*)(c->d_rad[phys] + off);
    if (rad_bytes) *rad_bytes = n * 16;
    return RT_OK;
}
/* Second lane for arbitrary calls: between rt_lane(ctx, 1) and rt_lane(ctx, 0) every enqueue of this
 * context goes to the second stream (ordered after rt_frame_stage_begin / _fork, joined by
 * rt_frame_stage_end) — e.g. the halo marks of the NEXT frame beside this frame's passes. */
int rt_lane(rt_ctx* c, int second)
{
    RT_CHECK_CTX(c);
    if (second)
    {
        if (c->lane_saved) RT_FAIL(c, RT_ERR_STATE, "rt_lane(1) twice");
        Launch lane;
        const int rc = second_lane(c, lane);
        if (rc != RT_OK) return rc;
        c->lane_main = c->stream;
        c->lane_timing = c->timing;
        c->stream = lane.stream;
        c->timing = lane.timed;
        c->lane_saved = true;
    }
    else if (c->lane_saved)
    {
        c->stream = c->lane_main;
        c->timing = c->lane_timing;
        c->lane_saved = false;
    }
    return RT_OK;
}

int rt_ray_count(rt_ctx* c, uint64_t* rays, uint64_t* shaded_pixels)
{
    RT_CHECK_CTX(c);
    if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "no G-buffer yet");
    RT_HIP(c, hipMemsetAsync(c->d_counter, 0, 8, c->stream));
    k_count_shaded<<<launch_grid(c, whole_launch(c)), BLOCK, 0, c->stream>>>(make_params(c, whole_launch(c), 0, 0), c->gbuf.g1, c->d_counter);
    RT_HIP(c, hipGetLastError());
    unsigned long long shaded = 0;
    RT_HIP(c, hipMemcpyAsync(&shaded, c->d_counter, 8, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t n = (uint64_t)c->W * (uint64_t)(c->row_end - c->row_begin);
    uint64_t per_shaded = 1; /* resolve (10_restir_di.cu:443-444) */
    if (c->opt.use_visibility_reuse) per_shaded += 1; /* :129-130 */
    uint64_t merged = 0;
    if (c->opt.use_shadowed_target_function)
    {
        /* p-hat of the candidate (:115-118), two of the temporal step (:195-199, :224-227), and per
         * spatial pass one per shaded pixel (:375-378) plus one per neighbour that reaches the target
         * function (:346-350). The latter is counted by replaying the passes' RNG against the shaded
         * bits of the last frame (any reservoir buffer of that frame carries them). */
        per_shaded += 1 + (c->opt.use_temporal_resampling ? 2 : 0);
        if (c->opt.use_spatial_resampling)
        {
            per_shaded += (uint64_t)c->opt.spatial_resampling_passes;
            unsigned long long* d = nullptr;
            RT_HIP(c, hipMalloc(&d, 24));
            RT_HIP(c, hipMemsetAsync(d, 0, 24, c->stream));
            for (int k = 0; k < c->opt.spatial_resampling_passes; ++k)
            {
                /* halo rows: G-buffer flags if the neighbours' were exchanged for this frame, else the records */
                const bool g1_ok = (c->row_begin == c->lrow0 || c->halo_flags_epoch[0] == c->epoch) && (c->row_end == c->lrow0 + c->lrows || c->halo_flags_epoch[1] == c->epoch);
                k_spatial_bytes<<<launch_grid(c, whole_launch(c)), BLOCK, 0, c->stream>>>(make_params(c, whole_launch(c), c->last_frame, k), c->gbuf.g1,
                                                                        c->d_rec[c->frame.res_map[RT_RES_TEMPORAL]], d, g1_ok);
            }
            RT_HIP(c, hipGetLastError());
            unsigned long long h[3] = {0, 0, 0};
            RT_HIP(c, hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, c->stream));
            RT_HIP(c, hipStreamSynchronize(c->stream));
            hipFree(d);
            merged = h[2];
        }
    }
    if (rays) *rays = n + per_shaded * shaded + merged;
    if (shaded_pixels) *shaded_pixels = shaded;
    return RT_OK;
}

/* shaded pixels (hit and not emissive: the ones that run RIS, reuse and shadow rays) of each owned
 * storage row of the current G-buffer, row_end - row_begin host counters */
/* BVH walks the build really performs (include/restir_rt.h) */
int rt_walk_stats_enable(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    if (on)
    {
        if (!c->d_walk) RT_HIP(c, hipMalloc(&c->d_walk, 4 * WALK_SLOTS * 8));
        /* on the context's stream, and complete before the call returns: a memset of device memory on the null stream may still be
         * running when the next launch on the (non-blocking) stream counts into it */
        RT_HIP(c, hipMemsetAsync(c->d_walk, 0, 4 * WALK_SLOTS * 8, c->stream));
        RT_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->walk_on = on != 0;
    /* a pipelined stage 0 enqueued before the switch carries the other setting: the next frame runs its own */
    drop_look_ahead(c);
    return RT_OK;
}
#ifdef RT_EXPERIMENTS
/* Experiments library only (not in include/restir_rt.h; tools/wave_timeline.py binds it by name). Arms the per-wavefront clock of
 * ONE kernel of the frame — 0 raycast, 1 generate_candidate, 2 spatial_resampling pass `pass`, 3 resolve, -1 off — or, with
 * `out` non-null, reads the 2 x n words the launches since then left (synchronises). Results never depend on it. */
int rt_exp_wave_clock(rt_ctx* c, int kernel, int pass, uint64_t* out, size_t n_words)
{
    RT_CHECK_CTX(c);
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    if (out)
    {
        if (!c->d_wave_clock) RT_FAIL(c, RT_ERR_STATE, "rt_exp_wave_clock: arm first");
        RT_HIP(c, hipMemcpy(out, c->d_wave_clock, std::min(n_words, c->wave_clock_words) * 8, hipMemcpyDeviceToHost)); /* the rest stays as the caller left it */
        return RT_OK;
    }
    /* one-wavefront workgroups over 8 x 8 tiles at most: every order's grid fits in twice the tile count */
    const size_t words = 16 * ((size_t)trace_grid(c, whole_launch(c)) + 1024) + 8 * (size_t)launch_grid(c, whole_launch(c)); /* k_raycast_quad: four workgroups per tile */
    if (kernel >= 0 && words > c->wave_clock_words)
    {
        if (c->d_wave_clock) hipFree(c->d_wave_clock);
        c->d_wave_clock = nullptr;
        RT_HIP(c, hipMalloc(&c->d_wave_clock, words * 8));
        c->wave_clock_words = words;
    }
    if (c->d_wave_clock) RT_HIP(c, hipMemset(c->d_wave_clock, 0, c->wave_clock_words * 8));
    c->wave_clock_kernel = kernel; c->wave_clock_pass = pass;
    drop_look_ahead(c);
    return RT_OK;
}
#endif
#ifdef RT_EXPERIMENTS
/* Experiments library only (tools/tile_lpt.py). Workgroup b of kernel 0 raycast / 1 generate_candidate (the one-launch stage 0 too) /
 * 3 resolve takes the tile workgroup perm[b] would have taken; perm must be a permutation of 0 .. n-1 that keeps b % 8 (checked), n =
 * the kernel's grid for the context's own rows; n = 0 removes it. Results never depend on it (every tile still runs exactly once). */
int rt_exp_tile_perm(rt_ctx* c, int kernel, const uint32_t* perm, size_t n)
{
    RT_CHECK_CTX(c);
    if (kernel != K_RAYCAST && kernel != K_GENERATE && kernel != K_RESOLVE) RT_FAIL(c, RT_ERR_ARG, "kernel 0, 1 or 3");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    if (c->d_tile_perm[kernel]) { hipFree(c->d_tile_perm[kernel]); c->d_tile_perm[kernel] = nullptr; c->tile_perm_n[kernel] = 0; }
    drop_look_ahead(c);
    if (n == 0) return RT_OK;
    if (!perm || n != (size_t)trace_grid(c, whole_launch(c))) RT_FAIL(c, RT_ERR_ARG, "the permutation must cover the kernel's %d workgroups", trace_grid(c, whole_launch(c)));
    std::vector<uint8_t> seen(n, 0);
    for (size_t b = 0; b < n; ++b)
    {
        if (perm[b] >= n || seen[perm[b]] || (perm[b] & 7u) != (b & 7u)) RT_FAIL(c, RT_ERR_ARG, "not an XCD-keeping permutation at %zu", b);
        seen[perm[b]] = 1;
    }
    RT_HIP(c, hipMalloc(&c->d_tile_perm[kernel], n * 4));
    RT_HIP(c, hipMemcpy(c->d_tile_perm[kernel], perm, n * 4, hipMemcpyHostToDevice));
    c->tile_perm_n[kernel] = n;
    return RT_OK;
}
#endif
int rt_walk_stats(rt_ctx* c, uint64_t out[16])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk, 16 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* r19. A switch of its own for the reason rt_gbuffer_reuse is one. Results never depend on it (occluder_hint.h). */
int rt_occluder_hints(rt_ctx* c, int on)
{
    RT_CHECK_CTX(c);
    c->hints_on = on != 0;
    /* a look-ahead enqueued under the other setting is not taken: the counters of rt_occluder_hint_stats follow the switch at once */
    drop_look_ahead(c);
    return RT_OK;
}
int rt_occluder_hint_stats(rt_ctx* c, uint64_t out[3])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk + 4 * WALK_HINTS, 3 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

/* r22. A switch of its own for the reason rt_gbuffer_reuse is one. Results never depend on it (neighbour_pick.h). */
int rt_neighbour_pick(rt_ctx* c, int mode)
{
    RT_CHECK_CTX(c);
    if (mode != PICK_EXACT && mode != PICK_FAST && mode != PICK_FORCE_SLOW) RT_FAIL(c, RT_ERR_ARG, "rt_neighbour_pick: mode must be 0, 1 or 2");
    c->pick_mode = mode;
    return RT_OK;
}
int rt_neighbour_pick_stats(rt_ctx* c, uint64_t out[2])
{
    RT_CHECK_CTX(c);
    if (!out) return RT_ERR_ARG;
    if (!c->d_walk) RT_FAIL(c, RT_ERR_STATE, "rt_walk_stats_enable first");
    int rc = rt_sync(c);
    if (rc != RT_OK) return rc;
    RT_HIP(c, hipMemcpy(out, c->d_walk + 4 * WALK_PICKS, 2 * 8, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_row_shaded(rt_ctx* c, uint32_t* counts)
{
    RT_CHECK_CTX(c);
    if (!counts) return RT_ERR_ARG;
    if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "no G-buffer yet");
    const int rows = c->row_end - c->row_begin;
    uint32_t* d = nullptr;
    RT_HIP(c, hipMalloc(&d, (size_t)rows * 4));
    RT_HIP(c, hipMemsetAsync(d, 0, (size_t)rows * 4, c->stream));
    k_row_shaded<<<rows, BLOCK, 0, c->stream>>>(c->W, c->row_begin - c->lrow0, c->gbuf.g1, d);
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(counts, d, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(d);
    return RT_OK;
}

/* visibility-reuse rays the last fused frame actually walked (rt_tuning key 11): the candidates that survived the
 * temporal merge. Synchronises the stream. With key 11 = 0 or outside rt_frame every shaded pixel walks one. */
int rt_visibility_rays_walked(rt_ctx* c, uint64_t* walked)
{
    RT_CHECK_CTX(c);
    if (!walked) return RT_ERR_ARG;
    if (!c->d_visq_count) RT_FAIL(c, RT_ERR_STATE, "no fused frame with deferred visibility rays has run");
    unsigned int h[2] = {0u, 0u};
    RT_HIP(c, hipMemcpyAsync(h, c->d_visq_count, 8, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->aux_stream) RT_HIP(c, hipStreamSynchronize(c->aux_stream));
    *walked = (uint64_t)h[0] + (uint64_t)h[1];
    return RT_OK;
}

int rt_spatial_bytes(rt_ctx* c, int frame, int pass, int in, uint64_t* bytes, uint64_t* accepted)
{
    RT_CHECK_CTX(c);
    NEED_RES(c, in);
    if (!c->gbuf.valid) RT_FAIL(c, RT_ERR_STATE, "no G-buffer yet");
    unsigned long long* d = nullptr;
    RT_HIP(c, hipMalloc(&d, 24));
    RT_HIP(c, hipMemsetAsync(d, 0, 24, c->stream));
    k_spatial_bytes<<<launch_grid(c, whole_launch(c)), BLOCK, 0, c->stream>>>(make_params(c, whole_launch(c), frame, pass), c->gbuf.g1, c->d_rec[c->frame.res_map[in]], d);
    RT_HIP(c, hipGetLastError());
    unsigned long long h[2] = {0, 0};
    RT_HIP(c, hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(d);
    if (bytes) *bytes = h[0];
    if (accepted) *accepted = h[1];
    return RT_OK;
}

/* ---- trace modes (enum rt_trace_mode_id): ONE row per mode holds what rt_trace_closest and rt_trace_stats launch in it ---- */
typedef hipError_t (*TraceLaunch)(rt_ctx* c, const float* d_rays, uint32_t n, void* d_out);
/* name = one launch of a ray-list kernel in workgroups of `threads` over `rays` rays; out_t = float (hits) or uint32_t (counters) */
#define TRACE_LAUNCH(name, out_t, threads, rays, ...) \
    static hipError_t name(rt_ctx* c, const float* d_r, uint32_t n, void* d_o) \
    { __VA_ARGS__<<<(n + (rays) - 1) / (rays), threads, 0, c->stream>>>(make_scene(c), d_r, (int)n, (out_t*)d_o); return hipGetLastError(); }
#ifdef RT_EXPERIMENTS
#define RT_EXP(launch) launch
static hipError_t trace_queue(rt_ctx* c, const float* d_r, uint32_t n, void* d_h) /* both queue modes: closest / any hit */
{
    unsigned int* d_head = (unsigned int*)c->d_counter;
    if (hipError_t e = hipMemsetAsync(d_head, 0, 8, c->stream)) return e;
    const int grid = 256 * 6; /* persistent: 6 workgroups per CU (24 KB LDS each) */
    if (c->trace_mode == RT_TRACE_QUEUE_CLOSEST) k_trace_queue<false><<<grid, BLOCK, 0, c->stream>>>(make_scene(c).wide, d_r, (int)n, (float*)d_h, d_head);
    else k_trace_queue<true><<<grid, BLOCK, 0, c->stream>>>(make_scene(c).wide, d_r, (int)n, (float*)d_h, d_head);
    return hipGetLastError();
}
#else
#define RT_EXP(launch) nullptr /* an A/B form of librestir_rt_exp.so */
#endif
TRACE_LAUNCH(trace_wide, float, 256, 256, k_trace_closest<0>)
TRACE_LAUNCH(trace_wide_any, float, 256, 256, k_trace_closest<0, true>)
TRACE_LAUNCH(trace_occluded_ws, float, TRACE_BLOCK, TRACE_BLOCK, k_trace_anyhit<true>)
TRACE_LAUNCH(trace_occluded_lane, float, TRACE_BLOCK, TRACE_BLOCK, k_trace_anyhit<false>)
#ifdef RT_EXPERIMENTS
TRACE_LAUNCH(trace_closest_quad, float, TRACE_BLOCK, 16, k_trace_closest_quad)
TRACE_LAUNCH(trace_binary, float, 256, 256, k_trace_closest<1>)
#endif
TRACE_LAUNCH(stats_ws, uint32_t, TRACE_BLOCK, TRACE_BLOCK, k_trace_stats_ws)
TRACE_LAUNCH(stats_wide, uint32_t, 256, 256, k_trace_stats<0>)
TRACE_LAUNCH(stats_wide_any, uint32_t, 256, 256, k_trace_stats<0, true>)
#ifdef RT_EXPERIMENTS
TRACE_LAUNCH(stats_binary, uint32_t, 256, 256, k_trace_stats<1>) /* also counts the modes that have no counting kernel of their own */
#endif
struct TraceRow
{
    int mode;
    TraceLaunch closest; /* nullptr: this library does not carry the mode (rt_trace_mode: RT_ERR_UNSUPPORTED) */
    bool closest_binary; /* walks the binary tree, which only rt_scene_set builds: refuses after an rt_scene_update */
    TraceLaunch stats;   /* nullptr: this library has no counting kernel for the mode (rt_trace_stats: RT_ERR_UNSUPPORTED) */
    bool stats_binary;
};
static constexpr TraceRow TRACE_MODES[] = {
    {RT_TRACE_WIDE, trace_wide, false, stats_wide, false},
    {RT_TRACE_BINARY, RT_EXP(trace_binary), true, RT_EXP(stats_binary), true},
    {RT_TRACE_QUEUE_CLOSEST, RT_EXP(trace_queue), false, RT_EXP(stats_binary), true},
    {RT_TRACE_QUEUE_ANY, RT_EXP(trace_queue), false, RT_EXP(stats_binary), true},
    {RT_TRACE_WIDE_ANY, trace_wide_any, false, stats_wide_any, false},
    {RT_TRACE_OCCLUDED_WS, trace_occluded_ws, false, stats_ws, false},
    {RT_TRACE_OCCLUDED_LANE, trace_occluded_lane, false, RT_EXP(stats_binary), true},
    {RT_TRACE_CLOSEST_QUAD, RT_EXP(trace_closest_quad), false, RT_EXP(stats_binary), true},
};
static_assert(rows_in_order(TRACE_MODES, RT_TRACE_MODE_COUNT, &TraceRow::mode), "TRACE_MODES: one row per mode, row i = mode i");

#define RT_CHECK_BINARY_TREE(c, binary)                                                                                   \
    do { if ((binary) && (c)->bin_stale) RT_FAIL(c, RT_ERR_STATE, "trace mode %d walks the binary tree, which rt_scene_update does not refit", (c)->trace_mode); } while (0)
int rt_trace_closest(rt_ctx* c, const float* rays, uint32_t n, float* hits)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "no scene");
    const TraceRow& mode = TRACE_MODES[c->trace_mode];
    RT_CHECK_BINARY_TREE(c, mode.closest_binary);
    if (n == 0) return RT_OK;
    float *d_r = nullptr, *d_h = nullptr;
    RT_HIP(c, hipMalloc(&d_r, (size_t)n * 32));
    RT_HIP(c, hipMalloc(&d_h, (size_t)n * 16));
    RT_HIP(c, hipMemcpyAsync(d_r, rays, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    hipEvent_t e0, e1;
    RT_HIP(c, hipEventCreate(&e0));
    RT_HIP(c, hipEventCreate(&e1));
    RT_HIP(c, hipEventRecord(e0, c->stream));
    RT_HIP(c, mode.closest(c, d_r, n, d_h));
    RT_HIP(c, hipEventRecord(e1, c->stream));
    RT_HIP(c, hipMemcpyAsync(hits, d_h, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipEventElapsedTime(&c->last_trace_ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(d_r); hipFree(d_h);
    return RT_OK;
}
/* the work-sharing any-hit walk of mode RT_TRACE_OCCLUDED_WS, asked for the triangle it found: tri[i] = its index, -1 = not occluded */
int rt_trace_occluders(rt_ctx* c, const float* rays, uint32_t n, int32_t* tri)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "no scene");
    if (n == 0) return RT_OK;
    if (!rays || !tri) return RT_ERR_ARG;
    float* d_r = nullptr;
    int* d_t = nullptr;
    RT_HIP(c, hipMalloc(&d_r, (size_t)n * 32));
    RT_HIP(c, hipMalloc(&d_t, (size_t)n * 4));
    RT_HIP(c, hipMemcpyAsync(d_r, rays, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    k_trace_occluders<<<(n + TRACE_BLOCK - 1) / TRACE_BLOCK, TRACE_BLOCK, 0, c->stream>>>(make_scene(c), d_r, (int)n, d_t);
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(tri, d_t, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(d_r); hipFree(d_t);
    return RT_OK;
}
/* device time of the traversal kernel of the last rt_trace_closest call */
int rt_trace_time(rt_ctx* c, float* ms)
{
    RT_CHECK_CTX(c);
    if (ms) *ms = c->last_trace_ms;
    return RT_OK;
}

/* per ray: {BVH nodes visited, triangle tests} of the closest-hit traversal */
int rt_trace_stats(rt_ctx* c, const float* rays, uint32_t n, uint32_t* stats)
{
    RT_CHECK_CTX(c);
    if (!c->has_scene) RT_FAIL(c, RT_ERR_STATE, "no scene");
    const TraceRow& mode = TRACE_MODES[c->trace_mode];
    if (!mode.stats) RT_FAIL(c, RT_ERR_UNSUPPORTED, "trace mode %d has no counting kernel in this library (librestir_rt_exp.so counts it on the binary walk)", c->trace_mode);
    RT_CHECK_BINARY_TREE(c, mode.stats_binary);
    if (n == 0) return RT_OK;
    float* d_r = nullptr;
    uint32_t* d_s = nullptr;
    RT_HIP(c, hipMalloc(&d_r, (size_t)n * 32));
    RT_HIP(c, hipMalloc(&d_s, (size_t)n * 8));
    RT_HIP(c, hipMemcpyAsync(d_r, rays, (size_t)n * 32, hipMemcpyHostToDevice, c->stream));
    RT_HIP(c, mode.stats(c, d_r, n, d_s));
    RT_HIP(c, hipMemcpyAsync(stats, d_s, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(d_r); hipFree(d_s);
    return RT_OK;
}
/* BVH build knob (before rt_scene_set): fragment length of the triangle pre-split in median
 * triangle extents; 0 disables splitting. */
int rt_bvh_config(rt_ctx* c, float split_factor)
{
    RT_CHECK_CTX(c);
    if (!(split_factor >= 0.0f)) RT_FAIL(c, RT_ERR_ARG, "split_factor must be >= 0");
    c->bvh_split_factor = split_factor;
    return RT_OK;
}
/* ---- performance knobs (enum rt_tuning_key; results never depend on them): ONE row per key holds all rt_tuning and
 * rt_tuning_get know about it. Retiring an A/B form = narrowing its row's `accepts` and deleting its kernel. ---- */
struct TuneRow
{
    int key;
    const char* name;
    int& (*field)(rt_ctx*);
    bool (*accepts)(int);    /* the values of the key: anything else is RT_ERR_ARG */
    bool (*product)(int);    /* those librestir_rt.so carries: for anything else it answers RT_ERR_UNSUPPORTED, BEFORE it looks at
                                `accepts` (the rest are A/B forms measured and left off, which csrc/Makefile builds into
                                librestir_rt_exp.so with -DRT_EXPERIMENTS; the variant tests and tools load that one) */
    void (*on_set)(rt_ctx*); /* what else a new value invalidates; nullptr = nothing */
};
static bool any_value(int) { return true; }
static bool no_value(int) { return false; }
#define TUNE_ROW(KEY, FIELD, ...) {RT_TUNE_##KEY, "RT_TUNE_" #KEY, [](rt_ctx* c) -> int& { return c->FIELD; }, __VA_ARGS__}
static constexpr TuneRow TUNING[] = {
    TUNE_ROW(TILE_RAYCAST, tune_tile_mode[0], within<-1, 7>, any_value, nullptr),
    TUNE_ROW(TILE_GENERATE, tune_tile_mode[1], within<-1, 7>, any_value, nullptr),
    TUNE_ROW(TILE_SPATIAL, tune_tile_mode[2], within<-1, 7>, any_value, nullptr),
    TUNE_ROW(TILE_RESOLVE, tune_tile_mode[3], within<-1, 7>, any_value, nullptr),
    TUNE_ROW(SPATIAL_LDS, tune_spatial_lds, within<0, 160 * 1024>, any_value, nullptr),
    TUNE_ROW(BVH_BUILDER, bvh_builder, within<0, 3>, within<3, 3>, nullptr), /* before rt_scene_set; [exp] 0 LBVH, 1 host SAH, 2 PLOC + host top */
    TUNE_ROW(PT_WAVEFRONT, pt_wavefront, within<0, 2>, any_value, nullptr),
    TUNE_ROW(BVH_BFS_RECORDS, bvh_bfs_records, within<0, INT_MAX>, any_value, nullptr), /* before rt_scene_set */
    TUNE_ROW(SPATIAL_VARIANT, tune_spatial_variant, within<0, 4>, within<2, 2>, [](rt_ctx* c) { c->gbuf.shaded_bits_stale = true; }), /* [exp] gather, LDS-staged bits, software-pipelined, one-wavefront workgroups */
    TUNE_ROW(SPATIAL_WAVES, tune_spatial_waves, [](int v) { return v == 0 || v == -1 || (v >= 4 && v <= 6); },
             [](int v) { return v == -1 || v == RT_SPATIAL_GATHER_AUTO_WAVES; }, nullptr), /* [exp] the other register budgets of the pass */
    TUNE_ROW(PLOC_RADIUS, ploc_radius, within<1, 256>, no_value, nullptr), /* before rt_scene_set; [exp] builder 2 */
    TUNE_ROW(DEFER_VIS, tune_defer_vis, within<0, 1>, within<0, 0>, nullptr), /* [exp] deferred visibility queue */
    TUNE_ROW(RIS_PIPE, tune_ris_pipe, within<0, 1>, within<0, 0>, nullptr),   /* [exp] pipelined RIS loop form */
    TUNE_ROW(WS, tune_ws, within<-1, 1>, any_value, nullptr),
    TUNE_ROW(SPEC, tune_spec, within<-1, 2>, any_value,
             [](rt_ctx* c) { if (!use_next_raycast(c, c->timing)) c->ahead.valid = false; if (!use_next_generate(c, c->timing)) c->ahead.gen_valid = false; }),
    TUNE_ROW(STREAM, tune_stream, within<0, 1>, within<0, 0>, nullptr), /* [exp] resolve as a stream */
    TUNE_ROW(WS_PRIMARY, tune_ws_primary, within<-1, 2>, [](int v) { return v != 2; }, nullptr), /* [exp] 2 = four lanes per primary ray */
    TUNE_ROW(TAIL, tune_tail, within<-1, 1>, any_value, nullptr),
    TUNE_ROW(MARK_QUICK, tune_mark_quick, within<0, 1>, any_value, nullptr),
    TUNE_ROW(MARK_WINDOW, tune_mark_window, within<0, 1>, any_value, nullptr),
    TUNE_ROW(FUSE_TONEMAP, tune_fuse_tonemap, within<0, 1>, any_value, nullptr),
    TUNE_ROW(MARK_CACHE, tune_mark_cache, within<0, 1>, any_value, [](rt_ctx* c) { c->mark_bits_epoch = 0; }),
    TUNE_ROW(SPEC_FREE, tune_spec_free, within<-1, 1>, any_value, drop_look_ahead),
    TUNE_ROW(FUSE_FINAL, tune_fuse_final, within<-1, 2>, within<INT_MIN, 0>, nullptr), /* [exp] last pass + resolve in one kernel */
    TUNE_ROW(HALF_RAYCAST, tune_half_raycast, within<0, 1>, within<0, 0>, nullptr), /* [exp] half-density raycast with helper lanes */
    TUNE_ROW(FUSE_RAYCAST, tune_fuse_raycast, within<-1, 1>, any_value, nullptr),
    TUNE_ROW(MARK_SPLIT, tune_mark_split, within<0, 1>, any_value, nullptr),
    TUNE_ROW(AO_LAYOUT, tune_ao_layout, within<0, 1>, any_value, nullptr),
    TUNE_ROW(DN_LAYOUT, tune_dn_layout, within<0, 1>, any_value, nullptr),
};
static_assert(rows_in_order(TUNING, RT_TUNE_COUNT, &TuneRow::key), "TUNING: one row per key, row i = key i");

int rt_tuning(rt_ctx* c, int key, int value)
{
    RT_CHECK_CTX(c);
    if (key < 0 || key >= RT_TUNE_COUNT) RT_FAIL(c, RT_ERR_ARG, "bad tuning key/value %d/%d", key, value);
    const TuneRow& row = TUNING[key];
#ifndef RT_EXPERIMENTS
    if (!row.product(value))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_tuning %d (%s) = %d selects an A/B form that only librestir_rt_exp.so (built with -DRT_EXPERIMENTS) carries", key, row.name, value);
#endif
    if (!row.accepts(value)) RT_FAIL(c, RT_ERR_ARG, "bad tuning key/value %d (%s)/%d", key, row.name, value);
    row.field(c) = value;
    if (row.on_set) row.on_set(c);
    return RT_OK;
}
int rt_tuning_get(rt_ctx* c, int key, int* value)
{
    RT_CHECK_CTX(c);
    if (!value) return RT_ERR_ARG;
    if (key < 0 || key >= RT_TUNE_COUNT) RT_FAIL(c, RT_ERR_ARG, "bad tuning key %d", key);
    *value = TUNING[key].field(c);
    return RT_OK;
}
#ifndef RT_BUILD_ID
#define RT_BUILD_ID "unknown"
#endif
const char* rt_build_id(void) { return RT_BUILD_ID; }
/* which traversal rt_trace_closest / rt_trace_stats exercise: a row of TRACE_MODES (enum rt_trace_mode_id) */
int rt_trace_mode(rt_ctx* c, int mode)
{
    RT_CHECK_CTX(c);
    if (mode < 0 || mode >= RT_TRACE_MODE_COUNT) RT_FAIL(c, RT_ERR_ARG, "mode must be 0..7");
    if (!TRACE_MODES[mode].closest) RT_FAIL(c, RT_ERR_UNSUPPORTED, "trace mode %d (binary stackless walk / ray queue / four lanes per ray) is an A/B form of librestir_rt_exp.so", mode);
    c->trace_mode = mode;
    return RT_OK;
}

int rt_math_eval(rt_ctx* c, int fn, const float* in, uint32_t n, float* out)
{
    RT_CHECK_CTX(c);
    if (n == 0) return RT_OK;
    const size_t nin = (fn == 26 || fn == 33 || fn == 35) ? 2 : ((fn == 31 || fn == 32) ? 12 : ((fn == 36 || fn == 37) ? 3 : (fn == 38 ? 14 : (fn == 45 ? 5 : 1)))); /* floats per item */
    float *d_i = nullptr, *d_o = nullptr;
    RT_HIP(c, hipMalloc(&d_i, (size_t)n * 4 * nin));
    RT_HIP(c, hipMalloc(&d_o, (size_t)n * 4));
    RT_HIP(c, hipMemcpyAsync(d_i, in, (size_t)n * 4 * nin, hipMemcpyHostToDevice, c->stream));
    k_math_eval<<<(n + 255) / 256, 256, 0, c->stream>>>(fn, d_i, (int)n, d_o);
    RT_HIP(c, hipGetLastError());
    RT_HIP(c, hipMemcpyAsync(out, d_o, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    RT_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(d_i); hipFree(d_o);
    return RT_OK;
}

} /* extern "C" */
