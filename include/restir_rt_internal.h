/*
 * restir_rt_internal.h — the part of librestir_rt.so's C-ABI that is NOT the reference-facing boundary.
 *
 * include/restir_rt.h declares what a host of the reference's shape binds (context, scene, camera, options, one entry
 * point per reference kernel, rt_frame, rt_mg_*, upload / download, timing, ray count). This header declares what the
 * build's own clients use on top of it:
 *   - the native strip driver (csrc/strip_mg.cpp) and the Python checker schedule (cedec_2024_rt_amd/strips.py):
 *     rt_frame_stage_*, rt_halo_*, stream / lane / region hooks, the stand-in transports of rt_mg_create;
 *   - the measurement tools (tools/, bench.py): rt_walk_stats, rt_spatial_bytes, rt_tuning, rt_wire_delay, rt_build_ms ...;
 *   - the parity tests: rt_trace_closest (BVH == brute force), rt_math_eval (device == host bits).
 * Same conventions as restir_rt.h: plain pointers and sizes, 0 or an RT_ERR_* code, nothing aborts. Nothing here is
 * needed to render a frame; results never depend on any call of this header (rt_tuning keys are tested bit for bit).
 */
#ifndef RESTIR_RT_INTERNAL_H
#define RESTIR_RT_INTERNAL_H

#include "restir_rt.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RT_RES_PHYS = 16 /* reservoir-buffer argument = RT_RES_PHYS + physical index, see rt_frame_stage_input */ };

/* ---- context / camera / path-trace extras ---- */
int rt_set_stream_own(rt_ctx* ctx);                /* back to the context's own non-blocking stream (default) */
int rt_camera_pose(rt_ctx* ctx, float eye[3], float lookat[3]); /* the pose the interactive camera holds now */

int rt_path_trace_rays(rt_ctx* ctx, uint64_t* rays); /* raytrace() calls of the last launch */

/* ---- scene update: the counterpart of HIPRT's hiprtBuildGeometry with hiprtBuildOperationUpdate (a refit) ---- */
/* Replace triangles [first, first + count) of the current scene (same total count, same index order).
 * Afterwards every result equals what rt_scene_set on the full new array would give. The tree keeps its topology
 * (rt_bvh_info does not change) and gets new boxes (a refit on the device): a triangle's leaf gets the triangle's box, and
 * each box fragment the build cut out of a large triangle gets the box of its own piece of the moved triangle (the pieces
 * are kept in barycentric coordinates, so they follow any deformation and do not drift over repeated updates). What a
 * refit cannot repair is topology: geometry thrown far from where it was built leaves large inner boxes, rt_bvh_cost says
 * how large, and rebuilding with rt_scene_set is the caller's decision. The per-triangle tables, the light table
 * and rt_scene_info's light count follow the new triangles. Any frame enqueued after the call sees the new scene: the
 * state epoch changes and the speculative next-frame work is dropped; accumulation is left alone (pass clear_first).
 * Synchronises the context's streams as rt_scene_set does. No scene: RT_ERR_STATE; a span beyond the scene or a NULL
 * pointer with count > 0: RT_ERR_ARG; count == 0: nothing changes. The experiments library's binary-tree walks refuse
 * (RT_ERR_STATE) after an update until the next rt_scene_set. */
int rt_scene_update(rt_ctx* ctx, const rt_triangle* triangles, uint32_t first, uint32_t count);

/* ---- denoiser: a spatial edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with the variance-guided luminance weight of
 * SVGF (Schied et al. 2017) over the accumulation buffer of a whole-frame context (csrc/denoise_math.h pins the arithmetic) ---- */
typedef struct
{
    int32_t iterations;        /* 0..8, default 5 (steps 1, 2, 4, 8, 16) */
    float sigma_luminance;     /* > 0, default 4 */
    float sigma_plane;         /* > 0, default 1 */
    int32_t normal_power_log2; /* 0..10, default 7 (n.n' ^ 128) */
    int32_t variance_radius;   /* 0..3, default 3 (7 x 7) */
} rt_denoise_params;
enum
{
    RT_BUF_DENOISED = 6,      /* float4[W*H], accumulation layout: the denoised HDR image; download only */
    RT_BUF_DENOISE_GUIDE = 7  /* rt_visibility[W*H] of the guide's primary hits; download only */
};
/* Filters the accumulation buffer as it stands (after the frames enqueued before the call) with guides from one primary ray per
 * pixel of the current camera, writes RT_BUF_DENOISED and its tone-mapped image into RT_BUF_PIXELS. Pixels that are sky,
 * emissive or have accumulation w == 0 keep their accumulation value. Asynchronous on the context's stream: it waits for the
 * streams that may still write the accumulation buffer and whatever is enqueued after it is ordered behind it; it changes neither
 * the accumulation buffer, the reservoirs, the state epoch nor the look-ahead work. params NULL = defaults. No scene or camera,
 * or a download of the two buffers before the first call: RT_ERR_STATE; strip contexts: RT_ERR_UNSUPPORTED; a parameter out of
 * range: RT_ERR_ARG. rt_tuning key 28 picks the layout of the a-trous levels (0 per-lane gathers, 1 residue lattice in LDS): the
 * same results. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params);
/* device time of the last rt_denoise run while rt_timing_enable was on: ms[0] guide, [1] demodulation + variance, [2] the levels
 * before the last, [3] the last level (fused output), [4] the whole call */
int rt_denoise_timing(rt_ctx* ctx, float ms[5]);

/* ---- temporal denoiser: SVGF's reprojection and history (Schied et al. 2017) in front of rt_denoise's filter ---- */
typedef struct
{
    float alpha_color;   /* (0, 1], default 0.2 */
    float alpha_moments; /* (0, 1], default 0.2 */
} rt_denoise_temporal_params;
enum
{
    RT_BUF_DENOISE_HISTORY = 8 /* float4[W*H] {mu1, mu2, history length, lambda'} of the last rt_denoise_temporal call; download only.
                                  lambda' is rt_denoise_temporal_antilag's response: 0 unless that toggle is on */
};
/* rt_denoise's contract, for one frame of a sequence: the accumulation buffer as it stands is the new frame (call it once per
 * frame). Per pixel the demodulated value is blended with its history, reprojected from the previous call's guide and camera
 * (csrc/denoise_math.h pins the arithmetic); the variance is the history's where it is 4 frames or longer; rt_denoise's levels
 * follow and the first level's output is the next call's colour history. Writes RT_BUF_DENOISED, RT_BUF_PIXELS,
 * RT_BUF_DENOISE_GUIDE and RT_BUF_DENOISE_HISTORY. The history is the context's, allocated at the first call: rt_scene_set and
 * rt_denoise_temporal_reset empty it; camera changes, rt_options_set, rt_scene_update and rt_denoise calls keep it. The first call
 * after a reset equals rt_denoise with the same spatial parameters. Whole-frame contexts only (RT_ERR_UNSUPPORTED); NULL
 * parameters = defaults; out of range: RT_ERR_ARG; RT_BUF_DENOISE_HISTORY before the first call or after a reset: RT_ERR_STATE. */
int rt_denoise_temporal(rt_ctx* ctx, const rt_denoise_params* spatial, const rt_denoise_temporal_params* temporal);
int rt_denoise_temporal_reset(rt_ctx* ctx);
/* device time of the last rt_denoise_temporal run while rt_timing_enable was on: ms[0] guide, [1] reprojection + integration,
 * [2] variance, [3] the levels before the last, [4] the last level (fused output), [5] the whole call */
int rt_denoise_temporal_timing(rt_ctx* ctx, float ms[6]);
/* (r25) The temporal denoiser's history follows geometry moved by rt_scene_update (csrc/denoise_motion.h),
 * default off: with it off every byte and every launch is what it was without the call. Independent of rt_temporal_reprojection and
 * rt_temporal_motion (the denoiser always follows the camera); it shares the kept vertex positions of one earlier generation with
 * rt_temporal_motion (rt_temporal_motion_range): they are copied from the current ones, with an empty range, when the first of the
 * two toggles goes on, freed when the last goes off, and left as they are, range included, by a toggle that goes on while they
 * exist; rt_scene_set makes them anew while either is on. rt_denoise_temporal tags its history with the geometry generation and the
 * eye it was written under. rt_scene_update brings the kept vertices to the generation it ends when a consumer whose toggle is on
 * wrote a history since the last update (a reservoir buffer for rt_temporal_motion, the denoiser's history for this toggle), and
 * otherwise only grows the range: with this toggle alone, all updates between two rt_denoise_temporal calls are followed, whether or
 * not frames were rendered in between. A call is a followed call iff the toggle is on, a history exists, the kept vertices exist,
 * the history's generation is the one they describe, and that is not the current generation. In a followed call a participating
 * pixel whose triangle lies in the moved range looks its history up from the point its guide hit (u, v) had on the triangle's
 * previous vertices, with the normal it had toward the previous call's eye: reprojection and the validity test of the four taps run
 * on that point and normal (also where the two cameras have the same bytes), with the current pixel's footprint; everything else of
 * the call uses the current guide. Every other pixel, and every call that is not followed (a history older than the kept vertices,
 * which happens when the two consumers alternate: frame, update, denoise, update, frame), does what rt_denoise_temporal does
 * without the toggle: the camera only, never a wrong previous vertex. NaN or infinite previous vertices, a previous point behind or
 * outside the previous camera: no history, h = 1. Changes neither rt_state_epoch nor the look-ahead, nor any reservoir or history
 * buffer. Strip contexts: RT_ERR_UNSUPPORTED. Not an rt_tuning key: tuning keys never change results. */
int rt_denoise_temporal_motion(rt_ctx* ctx, int on);
/* the toggle, and whether the last rt_denoise_temporal call was a followed call; either pointer may be null, not both */
int rt_denoise_temporal_motion_get(rt_ctx* ctx, int* on, int* last_call_followed);
/* (r30) Anti-lag for the temporal denoiser (csrc/denoise_antilag.h), default off: with it off every byte and
 * every launch is what it was without the call. rt_denoise_temporal blends with alpha = max(alpha, 1 / h) and cannot tell that its
 * history no longer describes the lighting (a moved object's shadow on a wall that did not move). An adapted call is one with the
 * toggle on and a history (not the first call after a reset); followed calls of rt_denoise_temporal_motion count. In an adapted call
 * every participating pixel with a history compares, over the (2 radius + 1)^2 window of pixels that have a history and whose normal
 * is within n . n' >= 0.9 of its own, the summed luminance of the current demodulated frame (mc) with that of the reprojected history
 * (mh): lambda = |mc - mh| / (max(mc, mh) + floor * members), lambda' = clamp((lambda - gradient_lo) / (gradient_hi - gradient_lo),
 * 0, 1), and both alphas become alpha + (1 - alpha) lambda' before max(., 1 / h). The history length is unchanged.
 * RT_BUF_DENOISE_HISTORY's fourth component carries lambda' (0 without history, in calls that are not adapted, with the toggle off).
 * The cost in a static scene is real (a firefly in a dark window is a relative gradient of 1; the floor trades it against the
 * response): DESIGN.md section 19 has the numbers. Parameters out of range or not finite: RT_ERR_ARG (nothing changes). Strip
 * contexts: RT_ERR_UNSUPPORTED. Changes neither rt_state_epoch nor the look-ahead, nor any reservoir or history buffer, and needs no
 * reset. Not an rt_tuning key: tuning keys never change results. */
typedef struct
{
    int32_t radius;                  /* 1..4, default 4 */
    float gradient_lo, gradient_hi; /* 0 <= lo < hi, defaults 0.2 and 0.8 */
    float floor;                     /* >= 0, default 0.05 */
} rt_denoise_antilag_params;
int rt_denoise_temporal_antilag(rt_ctx* ctx, int on, const rt_denoise_antilag_params* params /* NULL = defaults */);
/* the toggle, its parameters, and whether the last rt_denoise_temporal call was an adapted call; any pointer may be null, not all */
int rt_denoise_temporal_antilag_get(rt_ctx* ctx, int* on, rt_denoise_antilag_params* params, int* last_call_adapted);
/* device ms of k_denoise_antilag in the last rt_denoise_temporal call, if that was a timed adapted call (else RT_ERR_STATE);
 * rt_denoise_temporal_timing's ms[1] covers the gather kernel and this one */
int rt_denoise_temporal_antilag_timing(rt_ctx* ctx, float* ms);

/* ---- rt_frame in stages ---- */
/* The same frame cut into stages for strip contexts (multi-GPU): stage 0 = [clear,] raycast,
 * generate_candidate(+temporal); stage k in 1..passes = spatial pass k-1; stage passes+1 = resolve,
 * tone_mapping, buffer renaming. Before stage k in 1..passes the caller must fill the halo rows of
 * the buffer rt_frame_stage_input(ctx, k, &p) names (use RT_RES_PHYS + p with rt_halo_pack/unpack). */
int rt_frame_stage(rt_ctx* ctx, int frame, int stage, int clear_first);
int rt_frame_stage_input(rt_ctx* ctx, int stage, int* physical_buffer);
/* Finer control for overlapping halo traffic with compute: rt_frame_stage == _begin, one _run over
 * all owned rows, _end. A caller may instead _run the boundary rows first, start sending them
 * (rt_frame_stage_output names the buffer being written), _run the interior rows, then _end. */
int rt_frame_stage_begin(rt_ctx* ctx, int frame, int stage, int clear_first);
int rt_frame_stage_run(rt_ctx* ctx, int frame, int stage, int row0, int row1);
int rt_frame_stage_run_part(rt_ctx* ctx, int frame, int stage, int part, int row0, int row1); /* stage 0: part 1 = [clear,] raycast, 2 = generate, 0 = both */
/* Second lane: the same as _run_part, on the context's second stream, beside what the
 * main stream does for this stage (interior rows next to boundary rows). It starts after all work
 * enqueued on the main stream at _begin or at the last _fork; _end joins it. The two lanes' rows must
 * be disjoint and the lane must not read halo rows that are still being received. */
int rt_frame_stage_fork(rt_ctx* ctx);
int rt_frame_stage_run_async(rt_ctx* ctx, int frame, int stage, int part, int row0, int row1);
/* the same over up to two disjoint row ranges in ONE launch per kernel (ranges: n x {row0,row1}, n <= 2;
 * lane 1 = second stream): a launch that fits the GPU in one round lasts as long as its slowest
 * wavefront, so a strip's two boundary bands are cheaper as one launch than as two */
int rt_frame_stage_run_ranges(rt_ctx* ctx, int frame, int stage, int part, int n, const int* ranges, int lane);
int rt_frame_stage_end(rt_ctx* ctx, int stage);
int rt_frame_stage_output(rt_ctx* ctx, int stage, int* physical_buffer);
/* ---- multi-GPU halo rows: pack/unpack `n_rows` storage rows starting at
 * global row `row0` of reservoir buffer `res` to/from a caller-provided DEVICE buffer of
 * rt_halo_bytes(ctx, n_rows) bytes (exchanged by the caller, e.g. RCCL send/recv). ---- */
size_t rt_halo_bytes(rt_ctx* ctx, int n_rows);
int rt_halo_pack(rt_ctx* ctx, int res, int row0, int n_rows, void* device_dst);
int rt_halo_unpack(rt_ctx* ctx, int res, int row0, int n_rows, const void* device_src);

/* Sparse halos: a strip only needs the neighbour records its own pixels will load. That set is every
 * neighbour its own rows pick that lies inside the image and is not the pixel itself, shaded or not:
 * the spatial kernels load a record before they know its shaded bit, which they take from the record.
 * The shaded bits enter only through the draws (a shaded neighbour consumes a third one), so the set
 * is a pure function of the RNG and the shaded bits; a bitmap holds exactly it, no bit more or less
 * ("the contract of a plan"). Bitmap of n_rows rows, nw = (n_rows*W+31)/32:
 * word 0 = count, words [1, 1+nw) = bit (row - row0)*W + x, pad bits 0, words [1+nw, 1+2nw) = exclusive
 * prefix of the per-word popcounts; nw = 0 is the count word alone. The RECEIVER marks them (rt_halo_mark: side 0 = strip
 * below, 1 = strip above; needs the neighbour's shaded flags in its G-buffer halo rows, exchanged
 * once per frame with rt_halo_flags_*), sends the bitmap (first 1 + (n_rows*W+31)/32 words; word 0 =
 * record count) to the owner, and the owner answers each pass with the marked records only
 * (rt_halo_pack_sparse after rt_halo_scan on the received bitmap; 80 bytes per record, bitmap order);
 * rt_halo_unpack_sparse scatters them into the halo rows. Same results as the dense calls. */
size_t rt_halo_bitmap_words(rt_ctx* ctx, int n_rows);
size_t rt_halo_flags_bytes(rt_ctx* ctx, int n_rows);
int rt_halo_flags_pack(rt_ctx* ctx, int row0, int n_rows, void* device_dst);
int rt_halo_flags_unpack(rt_ctx* ctx, int row0, int n_rows, const void* device_src);
int rt_halo_mark(rt_ctx* ctx, int frame, int first_pass, int n_passes, int side, void* device_bitmaps); /* n_passes bitmaps, back to back */
int rt_halo_scan(rt_ctx* ctx, int n_rows, int n_bitmaps, void* device_bitmaps);
int rt_halo_pack_sparse(rt_ctx* ctx, int res, int row0, int n_rows, const void* device_bitmap, void* device_dst);
int rt_halo_unpack_sparse(rt_ctx* ctx, int res, int row0, int n_rows, const void* device_bitmap, const void* device_src);
/* the same with both neighbours served by ONE launch each (the native strip driver: a strip's frame is a chain of small
 * launches): rt_halo_mark_sides marks side 0 and / or side 1 (NULL = no neighbour there; if both pointers lie in one
 * allocation, side 0 first and at most 1 MiB apart, everything from the first bitmap to the end of the last is cleared
 * by one memset); the _ranges calls pack / unpack up to two row ranges. */
int rt_halo_mark_sides(rt_ctx* ctx, int frame, int first_pass, int n_passes, void* device_bitmaps_side0, void* device_bitmaps_side1);
int rt_halo_pack_sparse_ranges(rt_ctx* ctx, int res, int n, const int* row0, const int* n_rows, const void* const* device_bitmaps, void* const* device_dsts);
int rt_halo_unpack_sparse_ranges(rt_ctx* ctx, int res, int n, const int* row0, const int* n_rows, const void* const* device_bitmaps, const void* const* device_srcs);

/* The same without pack / unpack launches (r03): the running spatial stage gathers halo records straight from the received
 * lists (per side: the need-bitmap the receiver marked + the list that arrived) and writes the records its neighbours marked
 * (give-bitmap) into the send lists as it produces them. Call between rt_frame_stage_begin(stage in 1..passes) and the _run
 * calls it applies to; rt_frame_stage_end clears it; NULL clears it. Same results as the separate calls. */
typedef struct
{
    const void* need_bitmap[2]; const void* recv_list[2]; /* side 0 = strip below, 1 = above; NULL = none */
    const void* give_bitmap[2]; void* send_list[2];
} rt_halo_fuse;
int rt_halo_fuse_set(rt_ctx* ctx, const rt_halo_fuse* fuse);

/* ---- hooks used by the native strip driver below (and usable by any other driver) ---- */
int rt_state_epoch(rt_ctx* ctx, uint64_t* epoch);   /* changes whenever camera, options, scene or an uploaded G-buffer change */
int rt_get_stream(rt_ctx* ctx, void** hip_stream);  /* the stream calls are enqueued on right now */
int rt_side_stream(rt_ctx* ctx, int which, void** hip_stream); /* which = 0: the tail stream (rt_tuning key 17); the strip driver marks its halo plans there */
/* n <= 8 device-to-device copies in ONE launch on the context's current stream: what the strip driver's stand-in transports
 * (LOCAL, MIRROR) move the parts of an exchange with, as one grouped ncclSend/ncclRecv is one launch */
int rt_copy_parts(rt_ctx* ctx, int n, const void* const* src, void* const* dst, const size_t* bytes);
/* RT_MG_TRANSPORT_WIRE_MODEL: a dependent delay on the context's current stream. phase 0 notes the GPU wall clock when the stream
 * reaches it; phase 1 holds the stream until `ns` after that note (slot 0..7). No host sleep, one sleeping wavefront. */
int rt_wire_delay(rt_ctx* ctx, int phase, int slot, unsigned long long ns);
int rt_geometry(rt_ctx* ctx, int* width, int* height, int* row_begin, int* row_end, int* halo);
/* device addresses of n_rows storage rows of a reservoir buffer: 64-B records and 16-B radiance side
 * records; dense halos travel from / into the buffers themselves */
int rt_res_region(rt_ctx* ctx, int res, int row0, int n_rows, void** rec, size_t* rec_bytes, void** rad, size_t* rad_bytes);
/* rt_lane(ctx, 1) .. rt_lane(ctx, 0): calls in between are enqueued on the context's second stream
 * (the lane of rt_frame_stage_run_async; joined by rt_frame_stage_end) */
int rt_lane(rt_ctx* ctx, int second);

/* ---- strip driver: partition helper, stand-in transports, lock-step stepping, statistics ---- */
/* rows of a strip its neighbours can reach (computed and sent first) and the rest; up to 2 ranges each */
int rt_mg_bands(const int* bounds, int world, int rank, int halo, int* boundary, int* n_boundary, int* interior, int* n_interior);
/* stand-in transports of rt_mg_create (RT_MG_TRANSPORT_RCCL = 0 is the product's) */
enum { RT_MG_TRANSPORT_LOCAL = 1, RT_MG_TRANSPORT_MIRROR = 2 /* a rank receives what it sent: one rank alone, for overhead measurements (results are not a frame) */,
       RT_MG_TRANSPORT_SHM = 3 /* N processes of one node through a POSIX shared-memory segment (arg = its name, the same string on every
                                  rank): host-staged and blocking, for exact multi-process runs where RCCL cannot go (N ranks on ONE GPU) */,
       RT_MG_TRANSPORT_RCCL_SELF = 4 /* MIRROR with the real thing on the chain (r04): one rank alone, a ONE-rank RCCL communicator, every
                                  exchange = the grouped ncclSend/ncclRecv of the RCCL transport with the true per-side message sizes, on the
                                  stream the RCCL transport uses, addressed to the rank itself — so overhead measurements on a 1-GPU box
                                  contain RCCL's launch and copy kernel (no xGMI wire time) */,
       RT_MG_TRANSPORT_WIRE_MODEL = 5 /* RCCL_SELF + the xGMI wire (r05): an exchange completes no earlier than
                                  max over the two neighbours (bytes to / from that neighbour) / RT_MG_WIRE_GBS (default 153 GB/s, one
                                  link per neighbour) + RT_MG_WIRE_LAT_US (default 5 us) after its data was ready on the stream — a
                                  dependent delay on the exchange's stream (rt_wire_delay), not a host sleep. What tools/strip_overhead.py
                                  reports as THE bound of an N-strip frame on one-GPU boxes. */,
       RT_MG_TRANSPORT_MIRROR_WIRE = 6 /* (r06) MIRROR + the same dependent delay: a copy launch per exchange, and the exchange completes no
                                  earlier than the modelled link allows after its data was ready. The other bracket of the bound: RCCL's
                                  one-rank self-send moves a 4K exchange at ~85 GB/s — slower than the 153-GB/s link it stands in for —
                                  so WIRE_MODEL charges a real peer transfer's time twice over; this transport charges the wire alone. */ };
const char* rt_mg_load_error(void);
int rt_mg_hub_create(int world, void** hub); /* LOCAL transport: mailbox of `world` contexts in ONE process (tests) */
int rt_mg_hub_destroy(void* hub);
/* the same frame in segments that end where an exchange was posted: LOCAL contexts are stepped in
 * lock-step (every rank's segment i before any rank's segment i+1); *more = 0 after the last one */
int rt_mg_frame_begin(rt_mg* mg, int frame, int clear_first);
int rt_mg_frame_step(rt_mg* mg, int* more);
int rt_mg_reset_stats(rt_mg* mg);
/* one-rank RCCL communicator sending `bytes` to itself through the grouped send/recv path (1-GPU boxes) */
int rt_mg_selftest_rccl(size_t bytes);

/* ---- measurement ---- */
/* visibility-reuse rays the last rt_frame actually walked (rt_tuning key 11; the reference count of rt_ray_count does
 * not change): candidates that survived the temporal merge */
int rt_visibility_rays_walked(rt_ctx* ctx, uint64_t* walked);
/* BVH walks the build really performs, next to the rays the reference traces (r04; common/raytrace.hpp:18-52 is what a
 * "ray" costs the reference: every raytrace() call is a traversal). While enabled, the frame's default kernels count per
 * kernel slot k = 0 raycast, 1 generate_candidate(+temporal_resampling), 2 spatial_resampling (shadowed target function; the
 * unshadowed pass traces nothing), 3 resolve:
 *   out[4k + 0] rays the reference traces in that kernel,  out[4k + 1] of them walked through the BVH here,
 *   out[4k + 2] settled by the one-triangle self-occlusion test (the ray starts below its own surface),
 *   out[4k + 3] not evaluated: the answer is known from the own-visibility flags of an earlier kernel of the frame, or
 *               cannot be observed (visibility-reuse ray of a candidate that lost the temporal merge, weight-0 neighbours).
 * Counters accumulate over launches since rt_walk_stats_enable(ctx, 1) (which zeroes them; both calls synchronise). Covered:
 * k_raycast, the fused work-sharing generate_candidate of rt_frame (unshadowed), k_resolve, the <= 5-neighbour shadowed
 * spatial pass; other variants (rt_tuning A/B forms, shadowed candidates) leave their slot untouched. Results and timing
 * of a frame do not depend on it beyond a few atomics per wavefront; bench.py measures with it off. */
int rt_walk_stats_enable(rt_ctx* ctx, int on);
int rt_walk_stats(rt_ctx* ctx, uint64_t out[16]);
/* whether stage 0 of the last staged frame (rt_frame) ran as ONE launch — primary ray + candidates + temporal merge, rt_tuning
 * key 25 — on the context's stream. rt_timing then reports that launch as ms[2] and ms[1] is the empty bracket where the
 * raycast launch would have been (bench.py: `kernel_ms.stage0`). A look-ahead stage 0 (key 14) does not count. A frame that reuses
 * its G-buffer (rt_gbuffer_reuse) answers what a tracing frame would under the current tuning: its stage 0 on the stream is the
 * candidates' launch and ms[1] the empty bracket in either form. */
int rt_stage0_one_launch(rt_ctx* ctx, int* one_launch);
/* (r13) The primary ray of a pixel has no jitter and no frame number in it, so the G-buffer (RT_BUF_VISIBILITY and the two records
 * derived from it) is a function of camera, scene and image size. on = 1 (default on whole-frame contexts): stage 0 of a staged frame
 * (rt_frame, rt_frame_stage*) launches no primary rays while the current G-buffer set was traced over all owned rows, by stage 0 or
 * rt_raycast, under the current rt_state_epoch, and runs the candidates on that set; the look-ahead stage 0 (key 14) is then the
 * candidates alone. The first frame after rt_scene_set / rt_scene_update / a camera call / rt_options_set / an upload of
 * RT_BUF_VISIBILITY traces as before (an uploaded G-buffer is not a traced one). Bit-identical results: the skipped launch would
 * write the bytes the set holds. Always traced: rt_raycast, strip contexts, frames while rt_walk_stats_enable is on. on = 0: every
 * frame traces (A/B runs; tools that arm a clock or a permutation on the frame's raycast). on = 1 on a strip context:
 * RT_ERR_UNSUPPORTED. Not an rt_tuning key: tests/golden/tuning_matrix.json pins keys 29 and 30 as unknown and the table has one row
 * per key. */
int rt_gbuffer_reuse(rt_ctx* ctx, int on);
/* (r19) Occluder hints, default on: every pixel remembers the triangles that occluded its earlier candidate shadow rays, and the
 * candidates of a staged frame (rt_frame, rt_frame_stage*; whole-frame and strip contexts alike) test them, most recently used first,
 * before they walk the BVH. A remembered triangle is tested exactly, on its current vertices, with the ray's own origin, direction
 * and range: a hit is a hit of the walk, a miss leaves the walk to run, so results never depend on the switch nor on what the buffer
 * holds (csrc/occluder_hint.h). The buffer is made at the first staged frame, emptied by rt_scene_set, kept by rt_scene_update.
 * The per-kernel entry point rt_generate_candidate uses none. on = 0: A/B runs. Not an rt_tuning key, as rt_gbuffer_reuse. */
int rt_occluder_hints(rt_ctx* ctx, int on);
/* counted while rt_walk_stats_enable is on, zeroed by it: out[0] = candidate rays that had a remembered triangle to test, out[1] = rays
 * one of them settled (these count in rt_walk_stats' self_test of the generate_candidate slot: a one-triangle test, no walk),
 * out[2] = triangle tests made. Synchronises. */
int rt_occluder_hint_stats(rt_ctx* ctx, uint64_t out[3]);
/* (r22) The neighbour pick of the unshadowed spatial pass (k_spatial_coop; csrc/neighbour_pick.h). mode 1 (default): the two draws go
 * through the hardware's log2 / sqrt / sin / cos, and an interval guard proves per lane that the neighbour's integer pixel is the one
 * the portable functions give; the lanes it cannot clear ("near ties", about 0.1 %) run those functions. mode 0: the portable
 * functions on every lane (r01-r21). mode 2: the guard fails on every lane (the slow path through the fast form's control flow:
 * tests). The same bytes in every mode. Every other kernel that replays the pick (shadowed and unbiased passes, rt_halo_mark,
 * rt_spatial_bytes) computes the portable functions. Not an rt_tuning key, as rt_gbuffer_reuse. */
int rt_neighbour_pick(rt_ctx* ctx, int mode);
/* counted while rt_walk_stats_enable is on, zeroed by it: out[0] = neighbour picks k_spatial_coop made, out[1] = near ties among them
 * (mode 0 counts none, mode 2 all). Synchronises. */
int rt_neighbour_pick_stats(rt_ctx* ctx, uint64_t out[2]);
/* Unbiased spatial reuse, default off: every byte is then what it was without the call. While on,
 * rt_spatial_resampling, rt_frame and rt_frame_stage* run the spatial pass with the 1/Z normalisation of Bitterli et al. 2020 (Alg. 6)
 * whenever use_spatial_resampling = 1: Z counts only the contributors (the pixel and the merged neighbours) whose own target function
 * is positive at the selected light sample - geometry term from their G-buffer surface and, under use_visibility_reuse, one shadow
 * ray each - a neighbour's M is scaled by the rejection heuristics between the two G-buffer surfaces, and the record's visibility
 * flag is re-evaluated from the pixel itself, so that the record is valid as a neighbour in the next pass. Candidates, the temporal
 * merge, resolve and tone mapping are unchanged. Not built yet, RT_ERR_UNSUPPORTED at the launching call:
 * use_shadowed_target_function = 1, spatial_resampling_sample_count > 5. Strip contexts (and so rt_mg_frame): RT_ERR_UNSUPPORTED
 * from the toggle itself, their halo rows hold no traced G-buffer. The call changes rt_state_epoch, as rt_options_set does, and
 * touches no buffer. The temporal history needs no restart on either switch: it is saved before the spatial passes and never holds
 * a spatial pass's output. The [exp] spatial variants (rt_tuning keys 8 and 23) do not apply while the mode is on. rt_ray_count
 * keeps counting the reference's rays (none in an unshadowed pass). rt_walk_stats' spatial slot then reports 0 reference rays, the
 * rays walked, those the origin's own triangle settled and, as not_evaluated, the own rays an earlier kernel of the frame had
 * answered: the slot's sum is the pass's own rays, not the reference's. Not an rt_tuning key: tuning keys never change results. */
int rt_spatial_unbiased(rt_ctx* ctx, int on);
int rt_spatial_unbiased_get(rt_ctx* ctx, int* on);
/* Light selection of the ReSTIR candidates, default RT_LIGHTS_UNIFORM: every byte is then what it was without
 * the call. RT_LIGHTS_POWER: a candidate's emissive triangle is drawn with a probability proportional to area x luminance(Ke) from an
 * alias table built on the host at rt_scene_set / rt_scene_update (csrc/light_alias.h), with one more random number per candidate
 * (rv0, ra, bx, by, u); the pdf divided by is the one the table realises, so the estimate keeps its expectation. A property of the
 * context, set before or after the scene, on whole-frame and strip contexts alike (every strip of an rt_mg_frame must be given the
 * same mode); applies to rt_generate_candidate, rt_frame, rt_frame_stage* and rt_mg_frame, not to rt_path_trace. The call changes
 * rt_state_epoch and drops look-ahead work, touches no buffer and needs no new temporal history. Unknown mode: RT_ERR_ARG. A scene
 * in which no light has a positive finite area x luminance: RT_ERR_STATE from the launching call while the mode is RT_LIGHTS_POWER
 * and ris_sample_count > 0. Not an rt_tuning key: tuning keys never change results. */
enum { RT_LIGHTS_UNIFORM = 0 /* the reference's, default */, RT_LIGHTS_POWER = 1 };
int rt_light_sampling(rt_ctx* ctx, int mode);
int rt_light_sampling_get(rt_ctx* ctx, int* mode);
/* (r23) Temporal reuse that follows the camera (csrc/temporal_reproject.h), default off: every byte is then what
 * it was without the call. Every physical reservoir buffer carries the rt_raygen it was last written under: set by
 * rt_generate_candidate, rt_temporal_resampling, stage 0 and the spatial passes of a staged frame and rt_upload of a reservoir buffer
 * (each taking the current camera), copied by rt_save_temporal_reservoir and with the buffers as rt_frame rotates them, cleared by
 * rt_scene_set. While the mode is on, a temporal merge (rt_temporal_resampling, stage 0 of rt_frame / rt_frame_stage*) whose history
 * buffer carries a camera whose 36 bytes differ from the current ones takes, for every shaded pixel, the history of the previous
 * frame's pixel nearest to where the pixel's surface point projects in that camera, or Reservoir{} where there is none (behind the
 * previous camera, outside its image, NaN, or a previous pixel that was sky or emissive); the merge itself, its random numbers and
 * the rejection heuristics are the reference's. With equal bytes, or a buffer without a tag, the launches are the ones of the mode
 * off: a camera that stands still costs and computes what it did. Geometry moved by rt_scene_update is not followed (cameras only).
 * The call changes rt_state_epoch and drops look-ahead work, touches no buffer. Strip contexts (and so rt_mg_frame):
 * RT_ERR_UNSUPPORTED from the toggle, a previous pixel can lie in another strip. use_temporal_resampling = 0 makes it moot.
 * rt_temporal_resampling keeps refusing prev == inout (with a gather it would be a race). The [exp] stage-0 variants (rt_tuning keys
 * 11 and 12): RT_ERR_UNSUPPORTED at the launching call while the mode is on and the cameras differ. rt_ray_count keeps counting the
 * reference's rays. Not an rt_tuning key: tuning keys never change results. */
int rt_temporal_reprojection(rt_ctx* ctx, int on);
int rt_temporal_reprojection_get(rt_ctx* ctx, int* on);
/* the camera tag of RT_RES_* (tests): *has = 1 and *out = the rt_raygen, or *has = 0 and *out zeroed; either pointer may be null */
int rt_reservoir_camera(rt_ctx* ctx, int res, rt_raygen* out, int* has);
/* counted while rt_walk_stats_enable is on, zeroed by it: out[0] = shaded pixels merged by a reprojecting launch, out[1] = those that
 * found a valid history, out[2] = those among them whose history came from another pixel than their own. Synchronises. */
int rt_temporal_reprojection_stats(rt_ctx* ctx, uint64_t out[3]);
/* (r24) Temporal reuse that follows moved geometry (csrc/temporal_motion.h), default off, in effect only while
 * rt_temporal_reprojection is on: with it off every byte and every launch is what it was without the call. rt_scene_update counts a
 * geometry generation (0 after rt_scene_set); every physical reservoir buffer's tag also carries the generation and the eye it was
 * written under, set, copied and cleared with the camera tag. While the toggle is on the context keeps the vertex positions of one
 * earlier generation (rt_temporal_motion_range: which, and the covering range [lo, hi) of the spans updated since). rt_scene_update
 * brings them to the generation it ends when a reservoir buffer was written since the last update, and otherwise only grows the
 * range, so that several spans moved between two frames are all followed. A temporal merge whose history buffer carries exactly
 * that generation, and that generation is not the current one, is a motion launch: a shaded pixel whose triangle lies in [lo, hi)
 * takes the history of the previous frame's pixel that saw the point its surface point was at (the pixel's barycentrics on the
 * triangle's previous vertices, projected into the buffer's camera, also where that camera's bytes are the current one's), or
 * Reservoir{} where there is none, and the rejection heuristics compare that previous point, its normal and the previous eye with
 * the gathered record's origin. Every other pixel, and every merge that is no motion launch (an older history included), does
 * what rt_temporal_reprojection alone does. Not followed: moved emitters as samples, stale visibility flags, strips (the temporal
 * denoiser: rt_denoise_temporal_motion), changes of triangle count or order. The call changes rt_state_epoch and drops look-ahead work, touches no
 * reservoir buffer; going on it copies the current vertices (updates before it are not followed), going off it frees them. Strip
 * contexts: RT_ERR_UNSUPPORTED. The [exp] stage-0 variants (rt_tuning keys 11 and 12): RT_ERR_UNSUPPORTED at a motion launch. */
int rt_temporal_motion(rt_ctx* ctx, int on);
int rt_temporal_motion_get(rt_ctx* ctx, int* on);
/* the scene tag of RT_RES_* (tests): *has = 1, the geometry generation and the eye the buffer was written under, or *has = 0 and
 * zeros; any pointer may be null, not all */
int rt_reservoir_scene(rt_ctx* ctx, int res, uint64_t* generation, float eye[3], int* has);
/* the moved range and the generation the kept vertex positions describe (0, 0 and the current generation: nothing moved since) */
int rt_temporal_motion_range(rt_ctx* ctx, uint32_t* lo, uint32_t* hi, uint64_t* generation);
/* counted while rt_walk_stats_enable is on, zeroed by it: out[0] = shaded pixels merged by a motion launch, out[1] = those on a
 * triangle of the moved range, out[2] = those among them that found a valid history. Synchronises. */
int rt_temporal_motion_stats(rt_ctx* ctx, uint64_t out[3]);
/* (r31) The temporal merge normalised by 1/Z where its history comes from another pixel (DESIGN.md section 20;
 * csrc/temporal_unbiased.h), default off, in effect only while rt_temporal_reprojection is on: with it off every byte and every launch
 * is what it was without the call. An unbiased launch is a temporal merge (rt_temporal_resampling, stage 0 of rt_frame /
 * rt_frame_stage*) that is a reprojecting launch (its history buffer's camera tag differs from the current camera in its 36 bytes)
 * while the toggle is on; with equal bytes or no tag the launches are the ones of the toggle off, so a camera that stands still, the
 * look-ahead stage 0 and rt_gbuffer_reuse frames cost and compute what they did. The merge chain is the reference's (same draw, cap
 * and rejection heuristics); afterwards the gathered record counts in Z only if the selected sample y lies in its support: geometry
 * term > 0 from the record's origin and, under use_visibility_reuse, y visible from there (the record's flag if y is its own sample,
 * one shadow ray from its origin otherwise). W = w_sum / (Z p-hat), M stays the sum. Where the history's sample wins, the ray from the
 * pixel's own surface is walked in the merge (resolve finds its answer and does not walk it again), the stored visibility flag is its
 * answer, and the record's origin is the writer's surface whoever the sample came from. In a staged frame stage 0 is then two launches
 * on the frame's stream (the candidates without the merge, then k_temporal_unbiased), both inside rt_timing's ms[2]. The first unbiased
 * launch after frames rendered with the toggle off may meet an origin that travelled with its sample; nothing repairs it, it fades
 * with the M cap. RT_ERR_UNSUPPORTED: strip contexts (at the toggle); use_shadowed_target_function = 1 and the [exp] stage-0 variants
 * (rt_tuning keys 11 and 12), at an unbiased launch; rt_temporal_motion and this toggle both on (the second call refuses: the
 * history's origin would lie in geometry that no longer exists). The call changes rt_state_epoch and drops look-ahead work, touches no
 * buffer. rt_ray_count keeps counting the reference's rays. Not an rt_tuning key: tuning keys never change results. */
int rt_temporal_unbiased(rt_ctx* ctx, int on);
int rt_temporal_unbiased_get(rt_ctx* ctx, int* on);
/* counted while rt_walk_stats_enable is on, zeroed by it: out[0] = shaded pixels merged by unbiased launches, out[1] = those whose
 * history kept an M > 0 after the cap and the rejection heuristics, out[2] = those among them whose history was kept out of Z,
 * out[3] = rays walked from a history's origin. An unbiased launch is a reprojecting launch and counts in
 * rt_temporal_reprojection_stats as one, each shaded pixel once. Synchronises. */
int rt_temporal_unbiased_stats(rt_ctx* ctx, uint64_t out[4]);
/* (r32) History samples that follow moved emitters (csrc/light_follow.h), default off: with it off every byte and
 * every launch is what it was without the call. A history record stores its light sample as a world-space point, a normal and a
 * radiance; after rt_scene_update moved the emitter it still points at where the emitter was. While the toggle is on,
 * rt_scene_update(first, count) whose span holds an emissive triangle in the OLD array re-bases, before it overwrites anything, every
 * physical reservoir buffer whose light samples describe the generation the update ends (written under it, or re-based to it by the
 * update before: two updates with no frame between them are both followed, and an update whose span holds no emissive triangle in the old
 * array moves no emitter, so a buffer that was current stays current over it - a box moved before the lamp ends nothing; an older or
 * untagged buffer is left alone): a shaded
 * record with M > 0 whose sample lies on an old emissive triangle of the span (same normal and radiance bytes, on its plane and inside
 * it within measured tolerances; the nearest plane, then the lowest index) keeps every byte if the triangle's 60 bytes do not change,
 * becomes Reservoir{} (shaded bit kept) if the new triangle is non-emissive, degenerate or not finite, and is otherwise carried by
 * its barycentrics: new point, normal, luminance and radiance, ucw times the ratio of the areas, own-visibility word cleared; M,
 * w_sum, the origin and the visibility flag stay. No frame kernel changes. Independent of rt_temporal_reprojection,
 * rt_temporal_motion, rt_temporal_unbiased, rt_spatial_unbiased, rt_light_sampling and the target-function options. The toggle
 * changes rt_state_epoch and drops look-ahead work, touches no buffer. Strip contexts: RT_ERR_UNSUPPORTED. Not followed: visibility
 * flags, strips, the denoisers, lights whose count or order changes, older histories. Not an rt_tuning key. */
int rt_temporal_light_motion(rt_ctx* ctx, int on);
/* *on: the toggle; *last_update_rebased: buffers the last rt_scene_update re-based (0: none). Either pointer may be null, not both */
int rt_temporal_light_motion_get(rt_ctx* ctx, int* on, int* last_update_rebased);
/* totals since the toggle went on: out[0] = buffers re-based, out[1] = records examined (shaded, M > 0), out[2] = records located on a
 * triangle of the span, out[3] = records moved, out[4] = records emptied. RT_ERR_STATE before the toggle was ever on. Synchronises. */
int rt_temporal_light_motion_stats(rt_ctx* ctx, uint64_t out[5]);
/* device ms of the re-basing launches of the last rt_scene_update (0 if it re-based nothing) if the toggle and rt_timing_enable were
 * on during it, else RT_ERR_STATE */
int rt_temporal_light_motion_timing(rt_ctx* ctx, float* ms);
/* which locate path an update takes (tests, measurements): spans of at most direct_max old lights loop over them, larger ones query
 * the old tree; 0 = always the tree, negative = the default. Same bytes either way. */
int rt_temporal_light_motion_path(rt_ctx* ctx, int direct_max);
/* the alias table and the realised counts (thr / alias / K per light, light list order; any pointer may be null), for tests; n = the
 * scene's light count (RT_ERR_ARG otherwise); RT_ERR_STATE without a scene */
int rt_light_table(rt_ctx* ctx, uint32_t* thr, uint32_t* alias, uint64_t* K, uint32_t n);
/* Distance-aware light selection of the ReSTIR candidates (csrc/light_grid.h), default off: every byte is then
 * what it was without the call. On: the emissive triangles are grouped into min(clusters, lights) spatial clusters, a uniform grid of
 * cells_per_axis^3 cells over the scene's bounding box holds per cell an alias table over the clusters (cluster power over squared
 * distance), and a candidate draws a cluster from the table of its surface point's cell and a light from the cluster's own
 * power-proportional alias table, with three more random numbers per candidate than the reference (rv0, ra, rc, rb, bx, by, u). The pdf
 * divided by is the product of the two probabilities the tables realise, so the estimate keeps its expectation. Built on the host at
 * rt_scene_set, at an rt_scene_update whose span holds or held an emissive triangle or that moves the scene's bounds, and at this
 * call if a scene is present; while it is off nothing is built, kept or uploaded. cells_per_axis 1..32 and clusters 1..256 (suggested:
 * 16 and 64); cells_per_axis = 0 (clusters: anything) switches it off; anything else: RT_ERR_ARG, and nothing changes. While it is on
 * it decides the selection: rt_light_sampling's mode is kept, reported by its getter, and applies again when the grid goes off. A
 * property of whole-frame contexts (strips: RT_ERR_UNSUPPORTED), set before or after the scene; applies to rt_generate_candidate,
 * rt_frame and rt_frame_stage*, not to rt_path_trace. The call changes rt_state_epoch and drops look-ahead work, touches no reservoir
 * buffer and needs no new temporal history. A scene in which no light has a positive finite area x luminance: RT_ERR_STATE from the
 * launching call while the grid is on and ris_sample_count > 0. The experiments library's deferred and pipelined stage-0 forms
 * (rt_tuning keys 11 and 12) refuse it with RT_ERR_UNSUPPORTED. Tables that do not fit the device: RT_ERR_HIP, the grid stays as it was.
 * Not an rt_tuning key: tuning keys never change results. */
int rt_light_grid(rt_ctx* ctx, int cells_per_axis, int clusters);
/* the request as set (0, 0 = off) and the clusters the tables were built with (min(clusters, lights); 0 = no tables); any pointer may be null */
int rt_light_grid_get(rt_ctx* ctx, int* cells_per_axis, int* clusters, int* clusters_built);
/* wall time of the last table build (host tables and upload), ms; 0 before the first */
int rt_light_grid_build_ms(rt_ctx* ctx, float* ms);
/* The grid's tables, for tests; any pointer may be null. bounds: lo, hi, inv (3 floats each). Per light (n_lights = the scene's light
 * count): cluster_of in light list order; perm (the light at each sorted position) and, by sorted position, the clusters' alias slots
 * run_thr / run_alias (alias = a slot of the same cluster) with their realised counts run_K. run_start: clusters_built + 1 sorted
 * positions. Per cell slot (n_cell_slots = cells_per_axis^3 x clusters_built, cell-major): cell_thr / cell_alias / cell_K and
 * cell_prob, the binary32 probability the kernel multiplies by. cluster_of, run_start, the slots and cell_prob are read back from the
 * device; perm and the counts are the host's. Wrong counts: RT_ERR_ARG; no scene, or the grid off: RT_ERR_STATE. */
int rt_light_grid_table(rt_ctx* ctx, float bounds[9], uint32_t* cluster_of, uint32_t* perm, uint32_t* run_start, uint32_t* run_thr,
                        uint32_t* run_alias, uint64_t* run_K, uint32_t* cell_thr, uint32_t* cell_alias, uint64_t* cell_K, float* cell_prob,
                        uint32_t n_lights, uint32_t n_cell_slots);
/* (r36) Path-traced indirect light on top of the ReSTIR frame (csrc/indirect.h), default off: with bounces = 0
 * rt_frame issues the launches it issued without the call and nothing else. The frame's resolve writes the direct term of the primary
 * hit; with bounces = 1 .. 32 rt_frame (and the resolve stage of rt_frame_stage*, which must then run over all owned rows in one range:
 * RT_ERR_UNSUPPORTED otherwise) runs one more pass after resolve and before tone mapping, on the resolve's stream: every pixel whose
 * G-buffer entry is shaded starts a path at that surface with the random stream examples/08_nee gives the pixel for this frame number
 * (after the three draws of 08_nee's depth-0 light sample), and the path runs 08_nee's depth loop from depth 1 for `bounces`
 * iterations: closest hit, one uniformly picked light sample with one shadow ray, next direction; it ends on the sky or on an emissive
 * triangle without a contribution. Its radiance is added to RT_BUF_ACCUMULATION's RGB, the sample count .w stays; sky and emissive
 * pixels keep their bytes. Direct + indirect is what 08_nee estimates at max_depth = bounces + 1, term for term. The resolve kernel
 * then does not tone-map its own pixel (rt_tuning key 20 has no effect): tone mapping is a launch of its own behind the pass, and both
 * lie in rt_timing's ms[7], whose nine slots stay as they are. Light selection inside the bounces is uniform whatever
 * rt_light_sampling and rt_light_grid say. rt_ray_count keeps counting the reference's ReSTIR rays only. Other values of bounces:
 * RT_ERR_ARG; strip contexts: RT_ERR_UNSUPPORTED; a frame on a scene without lights while it is on: RT_ERR_STATE. The call changes
 * rt_state_epoch and touches no buffer. Not an rt_tuning key: tuning keys never change results. */
int rt_indirect(rt_ctx* ctx, int bounces);
int rt_indirect_get(rt_ctx* ctx, int* bounces);
/* the pass alone on the context's stream, for the kernel-by-kernel sequence between rt_resolve and rt_tone_mapping; bounces 1 .. 32.
 * RT_ERR_STATE without a traced G-buffer of the current camera and scene (rt_raycast, or a frame, since the last change of either)
 * and on a scene without lights; RT_ERR_UNSUPPORTED on strip contexts. rt_indirect itself changes rt_state_epoch, so it counts as such
 * a change: the pass takes its bounces as an argument and needs no toggle, and a caller who sets the toggle does so before rt_raycast. */
int rt_indirect_pass(rt_ctx* ctx, int frame, int bounces);
/* the last pass: out[0] = paths started (= shaded pixels), out[1] = raytrace()-equivalent rays (closest-hit + shadow), out[2] = paths
 * alive when its last bounce started. RT_ERR_STATE before the first pass. Synchronises. */
int rt_indirect_stats(rt_ctx* ctx, uint64_t out[3]);
/* device ms of the last pass if rt_timing_enable was on during it, else RT_ERR_STATE */
int rt_indirect_timing(rt_ctx* ctx, float* ms);
/* launches so far that traced primary rays over the context's rows: rt_raycast, stage-0 raycasts, the one-launch stage 0 and
 * look-ahead raycasts (counted when launched, taken or not). How the tests see reuse without timing anything. */
int rt_primary_launches(rt_ctx* ctx, uint64_t* n);
/* shaded pixels of each owned storage row (row_end - row_begin counters): the row cost of rt_mg_partition */
int rt_row_shaded(rt_ctx* ctx, uint32_t* counts);
/* ALGORITHMIC bytes (reference record sizes) of the spatial_resampling launch
 * (frame, pass) reading reservoir buffer `in`; `accepted` = neighbours that passed the
 * on-screen / not-self tests. Replays the RNG; independent of reservoir contents. */
int rt_spatial_bytes(rt_ctx* ctx, int frame, int pass, int in, uint64_t* bytes, uint64_t* accepted);
/* ---- BVH utilities (parity tests: BVH traversal == brute force) ----
 * rays: n x {ox,oy,oz, dx,dy,dz, tmin,tmax}; hits: n x {t,u,v, bits(index)}; host pointers.
 * Equal to brute force because the leaf boxes' pad, the quantiser's outward rounding and the margin of the accept predicate
 * together keep every box that holds a hit the intersector accepts (csrc/bvh_cull.h has the argument); held to it on random rays
 * (tests/test_gpu_parity.py) and on rays aimed at vertices, edges, box faces and duplicated triangles (tests/test_gpu_targeted_rays.py). */
int rt_trace_closest(rt_ctx* ctx, const float* rays, uint32_t n, float* hits);
/* per ray {nodes visited, triangle tests} of the same traversal (BVH quality diagnostics); for the
 * wide traversal the upper 16 bits of each word count the inner / leaf passes the ray's wavefront
 * executed while the ray was live (SIMT efficiency diagnostics) */
int rt_trace_stats(rt_ctx* ctx, const float* rays, uint32_t n, uint32_t* stats);
/* the work-sharing any-hit walk (mode RT_TRACE_OCCLUDED_WS, whatever rt_trace_mode says) asked for the triangle it found:
 * tri[i] = index of a triangle that occludes ray i - any of them, the walk's helpers race to report - or -1 if there is none */
int rt_trace_occluders(rt_ctx* ctx, const float* rays, uint32_t n, int32_t* tri);
/* BVH build knob, call before rt_scene_set: large triangles are pre-split into fragments no
 * longer than split_factor x (median triangle extent); 0 = no pre-split. Default 10. */
int rt_bvh_config(rt_ctx* ctx, float split_factor);
/* wide_height: levels of the 4-wide tree the kernels walk; a walk holds at most 3 stack entries per level */
int rt_bvh_info(rt_ctx* ctx, uint32_t* n_references, uint32_t* n_wide_records, uint32_t* wide_height);
/* SAH cost of the 4-wide tree as the walks see it: over all inner records and their occupied child slots,
 * half-area(child box decoded as the walk decodes it, lo + q * scale) / half-area(root box), summed in float64.
 * now: the tree as it stands; at_build: as rt_scene_set left it (equal to now until the first rt_scene_update).
 * Synchronises. No scene: RT_ERR_STATE; either pointer may be NULL. */
int rt_bvh_cost(rt_ctx* ctx, double* now, double* at_build);
int rt_build_ms(rt_ctx* ctx, float* ms); /* wall time of the last rt_scene_set (upload + tables + BVH build), synchronised */
/* which traversal rt_trace_closest / rt_trace_stats exercise. THE NUMBERS ARE FROZEN: tools, tests and every measurement log use
 * them. [exp] modes are A/B forms of librestir_rt_exp.so: the product library answers RT_ERR_UNSUPPORTED for them. Modes 4 .. 6
 * trace shadow rays (any hit): hits[i].index >= 0 iff occluded. rt_trace_stats answers RT_ERR_UNSUPPORTED in a mode for which
 * the library at hand has no counting kernel (the product library: mode 6). */
enum rt_trace_mode_id
{
    RT_TRACE_WIDE = 0,          /* 4-wide quantised BVH + LDS stack (what every frame kernel uses, default) */
    RT_TRACE_BINARY = 1,        /* [exp] binary LBVH + stackless trail (A/B measurements) */
    RT_TRACE_QUEUE_CLOSEST = 2, /* [exp] persistent lane-refill queue, closest hit */
    RT_TRACE_QUEUE_ANY = 3,     /* [exp] persistent lane-refill queue, any hit */
    RT_TRACE_WIDE_ANY = 4,      /* mode 0 with any-hit (shadow-ray) semantics */
    RT_TRACE_OCCLUDED_WS = 5,   /* shadow rays in one-wavefront workgroups as the frame kernels walk them, with the work-sharing
                                   walk (rt_trace_stats then returns its pass / steal counters); rays with tmax < 0 are lanes
                                   without a ray */
    RT_TRACE_OCCLUDED_LANE = 6, /* the same with one lane per ray */
    RT_TRACE_CLOSEST_QUAD = 7,  /* [exp] (r06) closest hit with FOUR LANES PER RAY, 16 rays per wavefront (closest_quad: what
                                   RT_TUNE_WS_PRIMARY = 2 gives the primary rays) */
    RT_TRACE_MODE_COUNT
};
int rt_trace_mode(rt_ctx* ctx, int mode);
int rt_trace_time(rt_ctx* ctx, float* ms); /* device ms of the last rt_trace_closest call's kernel */
/* Performance knobs; RESULTS NEVER DEPEND ON THEM (every key / value is tested bit for bit against the default). rt_tuning_get
 * returns the value a key holds, -1 meaning "auto" where a key has one. Keys marked [exp] select A/B forms that were measured and
 * left off: they are compiled only into librestir_rt_exp.so (csrc/Makefile, -DRT_EXPERIMENTS); the product library answers
 * RT_ERR_UNSUPPORTED for them. History and numbers of every key: docs/MEASUREMENT_LOG_*.md.
 * THE NUMBERS ARE FROZEN: bench.py, RT_TUNING=14=0,17=0, tools/profile_round.sh and every measurement log use them. A new key
 * takes the next number; a retired one keeps its number. */
enum rt_tuning_key
{
    /* ---- Launch geometry ---- */
    /* workgroup -> tile order of raycast (and rt_path_trace) / generate_candidate / spatial_resampling / resolve. Workgroup b runs
     * on XCD b % 8. 0, 1: XCD k takes ONE band of tile rows, row by row / column by column (r01-r04). r05, the XCDs
     * interleaved: 2, 3 = XCD k takes tile rows k, k + 8, ... (row by row / column by column), 4 = tile b (row-major) on XCD
     * b % 8, 5 = the same in stripes 32 tiles wide, 6, 7 = row-major runs of 4 / 16 tiles per XCD. -1 auto (default for all
     * four): tracing kernels 2 on whole frames, 4 on strips (a band costs what its part of the scene costs: raycast -14 %,
     * generate_candidate -9 %, resolve -12 %, an 8-rank 4K strip -7 %); the spatial pass 1 on whole frames and strips of
     * 400 rows or more (its +-87-px neighbour window must stay in one XCD's L2), 4 on shorter strips, 7 with the shadowed
     * target function (4.67 -> 3.83 ms per frame). profiles/r05_tile_interleave_ab.txt. */
    RT_TUNE_TILE_RAYCAST = 0,
    RT_TUNE_TILE_GENERATE = 1,
    RT_TUNE_TILE_SPATIAL = 2,
    RT_TUNE_TILE_RESOLVE = 3,
    /* extra LDS bytes per unshadowed spatial workgroup (round 1's occupancy throttle; default 0). */
    RT_TUNE_SPATIAL_LDS = 4,
    /* register budget of the unshadowed spatial pass in wavefronts per SIMD: -1 auto = 6 (default). [exp] 4, 5, 0 (= unbounded, 7). */
    RT_TUNE_SPATIAL_WAVES = 9,
    /* shadow rays of generate_candidate / resolve through the work-sharing any-hit walk: 1 always (default), 0 never, -1 only
     * for launches of about one generation of wavefronts. */
    RT_TUNE_WS = 13,
    /* primary rays through the work-sharing closest-hit walk: -1 auto = launches of about one generation of wavefronts, i.e.
     * strips (default), 0 never, 1 always (a whole frame's coherent 8 x 8 tiles gain nothing: 0.311 -> 0.318 ms); [exp] 2 (r06) =
     * four lanes per primary ray (k_raycast_quad: 16 rays per wavefront, each lane one child box of the 4-wide record, four
     * times the wavefronts: 78 -> 95 us for 135 rows, 228 -> 474 us for a whole frame; profiles/r06_quad_walk_ab.txt). */
    RT_TUNE_WS_PRIMARY = 16,
    /* [exp] (r05) raycast at half density: a wavefront carries 32 primary rays and 32 rayless lanes that only take work from
     * the others' stacks, twice the wavefronts (would a strip's one-generation launch finish sooner with two lanes per ray?
     * No: 80 -> 94 us for 135 rows, 269 -> 449 us for a whole frame; profiles/r05_half_raycast_ab.txt). Default 0. */
    RT_TUNE_HALF_RAYCAST = 24,

    /* ---- Scene (before rt_scene_set) ---- */
    /* BVH builder: 3 = on the device: pre-split, top-down binned SAH, 4-wide collapse; the host reads counters (default;
     * 11 ms for 212 k triangles). [exp] 0 = device LBVH + host collapse (r01), 1 = host binned SAH (the tree builder 3
     * reproduces, except below a node of more than 64 references with one common centroid: csrc/bvh_build_device.h; 230 ms), 2 = device PLOC + host SAH over the top 8 192 clusters. All feed the same walk. */
    RT_TUNE_BVH_BUILDER = 5,
    /* wide-BVH records emitted breadth-first before the collapse goes depth-first (default 2048; no measurable effect). */
    RT_TUNE_BVH_BFS_RECORDS = 7,
    /* [exp] PLOC search radius of builder 2 (default 16). */
    RT_TUNE_PLOC_RADIUS = 10,

    /* ---- Frame structure ---- */
    /* rt_path_trace: 0 one launch per frame (the reference's shape), 1 one launch per bounce over the compacted list of live
     * paths, 2 auto (default: per bounce for 09_ris). */
    RT_TUNE_PT_WAVEFRONT = 6,
    /* the NEXT frame's stage 0 on a stream of its own beside this frame's passes, exchanges and resolve: 0 never, 1 its
     * primary rays (second / third G-buffer set), 2 its generate_candidate + temporal_resampling too (the reference saves the
     * history before the passes, 10_restir_di.cpp:314-321), -1 auto = 2 (default; level 1 while rt_timing is enabled on a
     * whole-frame context). The next frame takes the results if frame number, camera, scene, options (rt_state_epoch) and
     * reservoir buffers are unchanged, and runs its own stage 0 otherwise. rt_sync waits for that stream too. */
    RT_TUNE_SPEC = 14,
    /* resolve + tone_mapping of a staged frame on a "tail" stream of their own: -1 auto = 1 on (default), 0 off. Off while
     * rt_timing is enabled. */
    RT_TUNE_TAIL = 17,
    /* (r05) stage 0 of the staged frame as ONE launch: the candidates' kernel traces the primary ray of its pixel first
     * (raycast needs nothing else, generate_candidate nothing but it; as two launches the second waits for the first one's
     * ramp-down): -1 auto = whole-frame contexts (default), 0 two launches, 1 also on strips. Applies to the product's fused
     * candidate kernel (temporal merge on, unshadowed target), also while rt_timing brackets the kernels (r06:
     * rt_stage0_one_launch); rt_raycast / rt_generate_candidate are always the two kernels. */
    RT_TUNE_FUSE_RAYCAST = 25,
    /* the staged frame's resolve kernel tone-maps the pixel it has just accumulated (common/kernels/common.cu:30-74 reads
     * nothing else): 1 (default), 0 = two launches as the reference. rt_resolve / rt_tone_mapping are always the two kernels. */
    RT_TUNE_FUSE_TONEMAP = 20,
    /* (r05) the look-ahead stage 0 (RT_TUNE_SPEC) of frame f+1 waits neither for the main stream (frame f took its own stage 0
     * from the look-ahead stream) nor for resolve(f-1): with three G-buffer sets and five reservoir buffers resolve(f-2) is the
     * last reader of what it overwrites. -1 auto = strips (default: rank 4 of 8 at 1080p 0.306 -> 0.287 ms), 0 never (r04's
     * dependencies), 1 always (a whole 1080p frame: 1.277 -> 1.296 ms). */
    RT_TUNE_SPEC_FREE = 22,

    /* ---- Spatial pass ---- */
    /* 2 = the wavefront fetches the 64 records of a round together, four lanes per 64-B record, as LDS-DMA loads that land
     * transposed in LDS, and writes its 64 records the same way (default, the only product form). [exp] 0 = one per-lane
     * gather per neighbour (r01), 1 = the tile's +-87-px window of shaded bits staged in LDS (r02), 3 = form 2 software-
     * pipelined over that window (r04: 0.152 against 0.1435 ms), 4 = form 2 as one-wavefront workgroups on 8 x 8 tiles (r05:
     * more wavefronts in flight, each slower: +1.3 %). */
    RT_TUNE_SPATIAL_VARIANT = 8,
    /* [exp] (r05) the LAST spatial pass + resolve in one kernel (k_spatial_resolve): 1 = with the pass's own stores, 2 = records
     * kept in registers (the pass's output buffer is NOT written), 0 / -1 = two kernels (default). Measured slower:
     * profiles/r05_fused_tail_ab.txt. */
    RT_TUNE_FUSE_FINAL = 23,

    /* ---- Candidates / resolve A/B forms ---- */
    /* [exp] visibility-reuse rays of the fused candidate kernel only for candidates that survive the temporal merge, through a
     * compacted queue (75 % survive in the bench scene: no gain). Default 0. */
    RT_TUNE_DEFER_VIS = 11,
    /* [exp] software-pipelined RIS loop form. Default 0. */
    RT_TUNE_RIS_PIPE = 12,
    /* [exp] resolve as a stream of persistent wavefronts (0.48 against 0.36 ms, r02). Default 0. */
    RT_TUNE_STREAM = 15,

    /* ---- Strips (multi-GPU) ---- */
    /* rt_halo_mark: rows more than 40 rows from a neighbour's region test the pass's first draws against a bound on the
     * neighbour distance before replaying log / sqrt / sincos: 1 (default), 0 = full replay. */
    RT_TUNE_MARK_QUICK = 18,
    /* rt_halo_mark collects a workgroup's marks in an LDS bitmap of its +-87-pixel window, one global atomic per non-zero
     * word: 1 (default; widths that are multiples of 32, reach <= 87 px, <= 3 passes per call), 0 = one atomic per mark. */
    RT_TUNE_MARK_WINDOW = 19,
    /* (r05) the shaded-bit rows RT_TUNE_MARK_WINDOW reads are built once per camera / scene / option epoch: 1 (default), 0 = in
     * front of every mark (r04). */
    RT_TUNE_MARK_CACHE = 21,
    /* (r06) rt_halo_mark as one workgroup per (tile, pass) instead of one per tile that replays the passes in series: 0
     * (default = r02-r05), 1. A strip's mark launch is half a generation of wavefronts and lasts as long as one thread's
     * chain of 3 x 5 neighbour replays - but it is not on the frame's critical chain and its total work stays the same:
     * measured +-1 % (profiles/r06_mark_split_ab.txt). */
    RT_TUNE_MARK_SPLIT = 26,

    /* ---- Ambient occlusion (rt_path_trace example 4 / 6) ---- */
    /* (r07) layout of the 64 occlusion rays per pixel: 0 (default) pixel-major, a lane walks its own pixel's rays back to back
     * and draws each when it starts it; 1 ray-major, the wavefront walks one pixel's 64 rays at a time (lane i from draw 3i
     * through the PCG jump-ahead). Same image either way (ambient occlusion). */
    RT_TUNE_AO_LAYOUT = 27,

    /* ---- Denoiser (rt_denoise, rt_denoise_temporal) ---- */
    /* layout of the a-trous levels: 0 per-lane gathers, 1 residue lattice in LDS. The same results. */
    RT_TUNE_DN_LAYOUT = 28,

    RT_TUNE_COUNT
};
int rt_tuning(rt_ctx* ctx, int key, int value);
/* the value a key holds now (measurement records name the builder / variants that were really used) */
int rt_tuning_get(rt_ctx* ctx, int key, int* value);
/* elementwise device evaluation of the portable math / IEEE div & sqrt (parity tests); fn ids as in
 * tests/test_portable_math.py; 31..35 (r04): the guarded shared-reciprocal divisions and square root of rt_device.h against
 * the compiler's (31 / 32: 12 floats per item = p0, n0, p1, n1; 33 / 35: 2 floats per item; results are XORs of bit patterns) */
int rt_math_eval(rt_ctx* ctx, int fn, const float* in, uint32_t n, float* out);
#ifdef __cplusplus
}
#endif
#endif /* RESTIR_RT_INTERNAL_H */
