"""csrc/history_provenance.h on the CPU: the tag of a history buffer (camera, geometry generation, eye, G-buffer serial) and the moved
range that rt_temporal_motion and rt_denoise_temporal_motion share.

The header is plain C++17 with no HIP include of its own, so g++ compiles what hipcc compiles. The program below holds, beside the
walk, a VERBATIM restatement of the statements the header replaced in restir_rt.hip (the fields of rt_ctx they touched under their old
names, the branches as they stood; HIP calls and rt_sync are stubs that write a log of device operations), and the few lines of
restir_rt.hip that now carry out what the header's transitions return. The walk applies EVERY sequence of DEPTH events, from a context
without a scene, to both and compares after every event the whole state, the log of device operations with their ranges, and the
followed-or-not decision of both consumers for every tag.

A second test drives the header beside the host rules of tests/denoise_motion_ref.py's MotionRef, the Python model the GPU tests of
rt_denoise_temporal_motion trust, over seeded random event sequences.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

DEPTH = 6  # 16 events: 16^6 = 16.8 M sequences, a few seconds; one more level is 16 times that

PROGRAM = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include "history_provenance.h"

using namespace rt;

#ifndef DEPTH
#define DEPTH 6
#endif

/* ---- the device, as far as the walk cares: a log of operations ---- */
enum { OP_SYNC = 1, OP_FREE = 2, OP_MALLOC = 3, OP_COPY = 4 };
struct Dev
{
    int n = 0;
    uint64_t op[15] = {};
    void push(uint64_t code, uint64_t a = 0, uint64_t b = 0)
    {
        if (n + 3 <= 15) { op[n] = code; op[n + 1] = a; op[n + 2] = b; }
        n += 3;
    }
};
static Dev* g_dev = nullptr;
static int g_bad_copy = 0; /* a copy whose source and destination are not the same triangles, or outside the 4 */
static float4 g_tv[12], g_tvp[12]; /* 4 triangles x 3 vertices: d_tv and d_tv_prev of BOTH sides */
typedef int hipError_t;
typedef int hipStream_t;
enum { hipSuccess = 0, hipMemcpyDeviceToDevice = 3, RT_ERR_HIP_ = -99 };
static hipError_t hipFree(void* p) { g_dev->push(OP_FREE, p != nullptr); return hipSuccess; }
static hipError_t hipMalloc(float4** p, size_t bytes) { *p = g_tvp; g_dev->push(OP_MALLOC, bytes); return hipSuccess; }
static hipError_t hipMemcpyAsync(float4* dst, const float4* src, size_t bytes, int, hipStream_t)
{
    const ptrdiff_t d = dst - g_tvp, s = src - g_tv;
    if (d != s || d < 0 || bytes % 48 != 0 || (size_t)d * 16 + bytes > sizeof(g_tvp)) ++g_bad_copy;
    g_dev->push(OP_COPY, (uint64_t)d, bytes);
    return hipSuccess;
}
#define RT_HIP(ctx, call) do { if ((call) != hipSuccess) return RT_ERR_HIP_; } while (0)

/* ---- the statements as they were (restir_rt.hip before history_provenance.h), restated verbatim ---- */
struct old_options { int use_temporal_resampling = 1; };
struct old_ctx
{
    rt_raygen rg = {};
    float eye[3] = {0.0f, 0.0f, 0.0f};
    struct { uint64_t serial = 0; } gbuf;
    int n_tris = 0;
    float4* d_tv = nullptr;
    bool has_scene = false;
    old_options opt;
    hipStream_t stream = 0;
    uint64_t rec_gserial[5] = {0, 0, 0, 0, 0};
    rt_raygen rec_rg[5] = {};
    bool rec_rg_has[5] = {false, false, false, false, false};
    bool reproject = true;
    uint64_t geo_gen = 0, tvp_gen = 0;
    uint64_t rec_gen[5] = {0, 0, 0, 0, 0};
    float rec_eye[5][3] = {};
    float4* d_tv_prev = nullptr;
    uint32_t mv_lo = 0, mv_hi = 0;
    bool res_dirty = false;
    bool motion = false;
    bool dn_motion = false, dt_dirty = false;
    rt_raygen dt_rg = {};
    uint64_t dt_gen = 0;
    float dt_eye[3] = {0.0f, 0.0f, 0.0f};
    bool dt_valid = false;
};
static int rt_sync(old_ctx*) { g_dev->push(OP_SYNC); return RT_OK; }
static void tag_camera(old_ctx* c, int phys)
{
    c->rec_rg[phys] = c->rg; c->rec_rg_has[phys] = true;
    c->rec_gen[phys] = c->geo_gen; memcpy(c->rec_eye[phys], c->eye, sizeof(c->rec_eye[phys]));
    c->res_dirty = true;
}
static void copy_camera(old_ctx* c, int phys, int src)
{
    c->rec_rg[phys] = c->rec_rg[src]; c->rec_rg_has[phys] = c->rec_rg_has[src];
    c->rec_gen[phys] = c->rec_gen[src]; memcpy(c->rec_eye[phys], c->rec_eye[src], sizeof(c->rec_eye[phys]));
}
/* history_motion, its decision */
static bool old_history_motion(const old_ctx* c, int prev_phys)
{
    if (!c->motion || !c->reproject || !c->opt.use_temporal_resampling || !c->rec_rg_has[prev_phys] || !c->d_tv_prev) return false;
    if (c->rec_gen[prev_phys] != c->tvp_gen || c->tvp_gen == c->geo_gen) return false;
    return true;
}
static bool old_dn_followed(const old_ctx* c)
{
    const bool followed = dn_motion_followed(c->dn_motion, c->dt_valid, c->d_tv_prev != nullptr, c->dt_gen, c->tvp_gen, c->geo_gen);
    return followed;
}
static int motion_rebase_all(old_ctx* c)
{
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    c->tvp_gen = c->geo_gen; c->mv_lo = 0; c->mv_hi = 0;
    if (!(c->motion || c->dn_motion) || !c->d_tv || c->n_tris <= 0) return RT_OK;
    RT_HIP(c, hipMalloc(&c->d_tv_prev, (size_t)c->n_tris * 48));
    RT_HIP(c, hipMemcpyAsync(c->d_tv_prev, c->d_tv, (size_t)c->n_tris * 48, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}
static int old_scene_set(old_ctx* c, uint32_t count)
{
    c->dt_valid = false; /* rt_denoise_temporal's history belongs to the old scene */
    for (int k = 0; k < 5; ++k) c->rec_rg_has[k] = false; /* ... and so do the reservoir buffers' camera tags: no reprojection into it */
    c->geo_gen = 0; c->tvp_gen = 0; c->mv_lo = 0; c->mv_hi = 0; c->res_dirty = false; c->dt_dirty = false; /* rt_temporal_motion: generations count from the new scene */
    /* free_scene */
    c->d_tv = nullptr;
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    const int n = (int)count;
    c->n_tris = n;
    if (n == 0) { c->has_scene = true; return RT_OK; }
    c->d_tv = g_tv; /* build_bvh */
    { const int rm = motion_rebase_all(c); if (rm != RT_OK) return rm; }
    c->has_scene = true;
    return RT_OK;
}
static int old_scene_update(old_ctx* c, uint32_t first, uint32_t count)
{
    if (!c->has_scene) return RT_ERR_STATE;
    if ((uint64_t)first + count > (uint64_t)c->n_tris) return RT_ERR_ARG;
    if (count == 0) return RT_OK;
    hipStream_t st = c->stream;
    if (c->d_tv_prev)
    {
        if ((c->motion && c->res_dirty) || (c->dn_motion && c->dt_dirty))
        {
            if (c->mv_hi > c->mv_lo)
                RT_HIP(c, hipMemcpyAsync(c->d_tv_prev + 3 * (size_t)c->mv_lo, c->d_tv + 3 * (size_t)c->mv_lo, (size_t)(c->mv_hi - c->mv_lo) * 48, hipMemcpyDeviceToDevice, st));
            c->tvp_gen = c->geo_gen;
            c->mv_lo = first; c->mv_hi = first + count;
        }
        else if (c->mv_hi > c->mv_lo) { c->mv_lo = std::min(c->mv_lo, first); c->mv_hi = std::max(c->mv_hi, first + count); }
        else { c->mv_lo = first; c->mv_hi = first + count; }
    }
    ++c->geo_gen;
    c->res_dirty = false;
    c->dt_dirty = false;
    return RT_OK;
}
static int old_temporal_motion(old_ctx* c, int on)
{
    const bool was = c->motion;
    c->motion = on != 0;
    if (c->motion == was) return RT_OK;
    if (c->dn_motion) return RT_OK; /* rt_denoise_temporal_motion holds d_tv_prev too: the buffer and the range stay as they are */
    /* launches in flight may read d_tv_prev */
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    return motion_rebase_all(c);
}
static int old_denoise_temporal_motion(old_ctx* c, int on)
{
    const bool was = c->dn_motion;
    c->dn_motion = on != 0;
    if (c->dn_motion == was) return RT_OK;
    c->dt_dirty = false; /* a history tagged while the toggle was off, or before this moment, re-bases nothing */
    if (c->motion) return RT_OK; /* the buffer is rt_temporal_motion's too: it stays, with its range */
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    return motion_rebase_all(c);
}
/* launch_generate, launch_spatial, the reservoir upload */
static void old_write_reservoir(old_ctx* c, int phys)
{
    c->rec_gserial[phys] = c->gbuf.serial;
    tag_camera(c, phys);
}
/* rt_temporal_resampling */
static void old_merge_in_place(old_ctx* c, int pi) { tag_camera(c, pi); }
/* rt_save_temporal_reservoir, rt_frame_stage_end */
static void old_copy_reservoir(old_ctx* c, int pd, int ps)
{
    c->rec_gserial[pd] = c->rec_gserial[ps];
    copy_camera(c, pd, ps);
}
/* the look-ahead take, rt_spatial_resampling after k_refresh_shaded */
static void old_refresh_bits(old_ctx* c, int phys) { c->rec_gserial[phys] = c->gbuf.serial; }
/* the end of rt_denoise_temporal */
static void old_denoise_temporal_end(old_ctx* c)
{
    c->dt_rg = c->rg;
    c->dt_gen = c->geo_gen; memcpy(c->dt_eye, c->eye, sizeof(c->dt_eye));
    if (c->dn_motion) c->dt_dirty = true;
    c->dt_valid = true;
}
static void old_denoise_temporal_reset(old_ctx* c)
{
    c->dt_valid = false; /* the next call reads none of the previous buffers */
}

/* ---- restir_rt.hip as it is now: the same entry points on the header ---- */
struct new_ctx
{
    rt_raygen rg = {};
    float eye[3] = {0.0f, 0.0f, 0.0f};
    struct { uint64_t serial = 0; } gbuf;
    int n_tris = 0;
    float4* d_tv = nullptr;
    bool has_scene = false;
    old_options opt;
    hipStream_t stream = 0;
    HistoryTag res_tag[5];
    bool reproject = true;
    MovedGeometry moved;
    float4* d_tv_prev = nullptr;
    HistoryTag dt_tag;
    bool dt_valid = false;
};
static int rt_sync(new_ctx*) { g_dev->push(OP_SYNC); return RT_OK; }
static void tag_reservoir(new_ctx* c, int phys, uint64_t gserial)
{
    c->res_tag[phys].write(c->rg, c->moved.geo_gen, c->eye, gserial);
    c->moved.tagged(FOLLOW_RESTIR);
}
static void tag_reservoir(new_ctx* c, int phys) { tag_reservoir(c, phys, c->gbuf.serial); }
static bool new_history_motion(const new_ctx* c, int prev_phys)
{
    const HistoryTag& t = c->res_tag[prev_phys];
    if (!c->reproject || !c->opt.use_temporal_resampling || !c->moved.follows(FOLLOW_RESTIR, t)) return false;
    return true;
}
static bool new_dn_followed(const new_ctx* c) { return c->moved.follows(FOLLOW_DENOISER, c->dt_tag, c->dt_valid); }
static bool scene_has_vertices(const new_ctx* c) { return c->d_tv && c->n_tris > 0; }
static int kept_vertices_replace(new_ctx* c, bool copy)
{
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    if (!copy) return RT_OK;
    RT_HIP(c, hipMalloc(&c->d_tv_prev, (size_t)c->n_tris * 48));
    RT_HIP(c, hipMemcpyAsync(c->d_tv_prev, c->d_tv, (size_t)c->n_tris * 48, hipMemcpyDeviceToDevice, c->stream));
    return RT_OK;
}
static int kept_vertices_toggled(new_ctx* c, KeptAction a)
{
    if (a == KEPT_NOTHING) return RT_OK;
    { const int rs = rt_sync(c); if (rs != RT_OK) return rs; }
    return kept_vertices_replace(c, a == KEPT_DRAIN_FREE_COPY);
}
static int new_scene_set(new_ctx* c, uint32_t count)
{
    c->dt_valid = false;
    for (HistoryTag& t : c->res_tag) t.has = false;
    const bool keep_vertices = c->moved.scene_set(count > 0);
    /* free_scene */
    c->d_tv = nullptr;
    hipFree(c->d_tv_prev);
    c->d_tv_prev = nullptr;
    const int n = (int)count;
    c->n_tris = n;
    if (n == 0) { c->has_scene = true; return RT_OK; }
    c->d_tv = g_tv; /* build_bvh */
    { const int rm = kept_vertices_replace(c, keep_vertices); if (rm != RT_OK) return rm; }
    c->has_scene = true;
    return RT_OK;
}
static int new_scene_update(new_ctx* c, uint32_t first, uint32_t count)
{
    if (!c->has_scene) return RT_ERR_STATE;
    if ((uint64_t)first + count > (uint64_t)c->n_tris) return RT_ERR_ARG;
    if (count == 0) return RT_OK;
    hipStream_t st = c->stream;
    const MovedUpdate mu = c->moved.update(first, count);
    if (mu.kind == MovedUpdate::REBASE && mu.hi > mu.lo)
        RT_HIP(c, hipMemcpyAsync(c->d_tv_prev + 3 * (size_t)mu.lo, c->d_tv + 3 * (size_t)mu.lo, (size_t)(mu.hi - mu.lo) * 48, hipMemcpyDeviceToDevice, st));
    return RT_OK;
}
static int new_temporal_motion(new_ctx* c, int on) { return kept_vertices_toggled(c, c->moved.toggle(FOLLOW_RESTIR, on != 0, scene_has_vertices(c))); }
static int new_denoise_temporal_motion(new_ctx* c, int on) { return kept_vertices_toggled(c, c->moved.toggle(FOLLOW_DENOISER, on != 0, scene_has_vertices(c))); }
static void new_denoise_temporal_end(new_ctx* c)
{
    c->dt_tag.write(c->rg, c->moved.geo_gen, c->eye, 0);
    c->moved.tagged(FOLLOW_DENOISER);
    c->dt_valid = true;
}

/* ---- the walk ---- */
enum Event
{
    EV_SCENE_4, EV_SCENE_0, EV_RES_ON, EV_RES_OFF, EV_DN_ON, EV_DN_OFF,
    EV_WRITE_0,   /* a launch writes reservoir buffer 0: tag and serial */
    EV_MERGE_1,   /* rt_temporal_resampling merges into buffer 1 in place: tag, the serial stays */
    EV_DN_CALL,   /* rt_denoise_temporal tags its history */
    EV_DN_RESET,  /* rt_denoise_temporal_reset */
    EV_COPY_0_1,  /* buffer 1 := buffer 0 */
    EV_BITS_1,    /* the shaded bits of buffer 1 refreshed: the serial alone */
    EV_UPDATE_0_1, EV_UPDATE_1_3, EV_UPDATE_3_4, EV_UPDATE_0_4,
    N_EVENTS
};
static const uint32_t SPAN[4][2] = {{0, 1}, {1, 2}, {3, 1}, {0, 4}}; /* {first, count} of [0,1) [1,3) [3,4) [0,4) */

static int old_apply(old_ctx* c, int e)
{
    switch (e)
    {
        case EV_SCENE_4: return old_scene_set(c, 4);
        case EV_SCENE_0: return old_scene_set(c, 0);
        case EV_RES_ON: return old_temporal_motion(c, 1);
        case EV_RES_OFF: return old_temporal_motion(c, 0);
        case EV_DN_ON: return old_denoise_temporal_motion(c, 1);
        case EV_DN_OFF: return old_denoise_temporal_motion(c, 0);
        case EV_WRITE_0: old_write_reservoir(c, 0); return RT_OK;
        case EV_MERGE_1: old_merge_in_place(c, 1); return RT_OK;
        case EV_DN_CALL: old_denoise_temporal_end(c); return RT_OK;
        case EV_DN_RESET: old_denoise_temporal_reset(c); return RT_OK;
        case EV_COPY_0_1: old_copy_reservoir(c, 1, 0); return RT_OK;
        case EV_BITS_1: old_refresh_bits(c, 1); return RT_OK;
        default: return old_scene_update(c, SPAN[e - EV_UPDATE_0_1][0], SPAN[e - EV_UPDATE_0_1][1]);
    }
}
static int new_apply(new_ctx* c, int e)
{
    switch (e)
    {
        case EV_SCENE_4: return new_scene_set(c, 4);
        case EV_SCENE_0: return new_scene_set(c, 0);
        case EV_RES_ON: return new_temporal_motion(c, 1);
        case EV_RES_OFF: return new_temporal_motion(c, 0);
        case EV_DN_ON: return new_denoise_temporal_motion(c, 1);
        case EV_DN_OFF: return new_denoise_temporal_motion(c, 0);
        case EV_WRITE_0: tag_reservoir(c, 0); return RT_OK;
        case EV_MERGE_1: tag_reservoir(c, 1, c->res_tag[1].gserial); return RT_OK;
        case EV_DN_CALL: new_denoise_temporal_end(c); return RT_OK;
        case EV_DN_RESET: c->dt_valid = false; return RT_OK;
        case EV_COPY_0_1: c->res_tag[1] = c->res_tag[0]; return RT_OK;
        case EV_BITS_1: c->res_tag[1].gserial = c->gbuf.serial; return RT_OK;
        default: return new_scene_update(c, SPAN[e - EV_UPDATE_0_1][0], SPAN[e - EV_UPDATE_0_1][1]);
    }
}
/* the same sequence with the two consumers' parts exchanged; -1: an event with no counterpart */
static int mirrored(int e)
{
    switch (e)
    {
        case EV_RES_ON: return EV_DN_ON;
        case EV_RES_OFF: return EV_DN_OFF;
        case EV_DN_ON: return EV_RES_ON;
        case EV_DN_OFF: return EV_RES_OFF;
        case EV_WRITE_0: case EV_MERGE_1: return EV_DN_CALL;
        case EV_DN_CALL: return EV_WRITE_0;
        case EV_DN_RESET: case EV_COPY_0_1: case EV_BITS_1: return -1;
        default: return e;
    }
}
static bool same_tag(const HistoryTag& t, const rt_raygen& rg, bool has, uint64_t gen, const float eye[3])
{
    return memcmp(&t.rg, &rg, sizeof(rg)) == 0 && t.has == has && t.gen == gen && memcmp(t.eye, eye, sizeof(t.eye)) == 0;
}
static bool same(const new_ctx& n, const old_ctx& o)
{
    for (int k = 0; k < 5; ++k)
        if (!same_tag(n.res_tag[k], o.rec_rg[k], o.rec_rg_has[k], o.rec_gen[k], o.rec_eye[k]) || n.res_tag[k].gserial != o.rec_gserial[k]) return false;
    if (!same_tag(n.dt_tag, o.dt_rg, n.dt_tag.has, o.dt_gen, o.dt_eye) || n.dt_valid != o.dt_valid) return false;
    if (o.dt_valid && !n.dt_tag.has) return false; /* a valid history was tagged: `has && valid` is `valid` */
    const MovedGeometry& m = n.moved;
    return m.geo_gen == o.geo_gen && m.kept_gen == o.tvp_gen && m.lo == o.mv_lo && m.hi == o.mv_hi && m.kept == (o.d_tv_prev != nullptr) &&
           n.d_tv_prev == o.d_tv_prev && m.on[FOLLOW_RESTIR] == o.motion && m.on[FOLLOW_DENOISER] == o.dn_motion &&
           m.dirty[FOLLOW_RESTIR] == o.res_dirty && m.dirty[FOLLOW_DENOISER] == o.dt_dirty && n.n_tris == o.n_tris && n.has_scene == o.has_scene &&
           n.d_tv == o.d_tv;
}

enum
{
    C_NODES, C_DIFFER, C_REBASE_NONEMPTY, C_REBASE_EMPTY, C_GROW_FROM_EMPTY, C_GROW_NONEMPTY, C_ON_WHILE_SHARED, C_LAST_OFF, C_TAG_OLDER,
    C_TAG_CURRENT, C_FOLLOWED_RES, C_FOLLOWED_DN, C_ASYMMETRY, C_BAD_COPY, C_LOG_OVERFLOW, N_COUNTS
};
static long long g_count[N_COUNTS];

struct State
{
    new_ctx n;
    old_ctx o, mirror;
};
static void step(const State& from, int depth)
{
    for (int e = 0; e < N_EVENTS; ++e)
    {
        State s = from;
        /* the camera and the G-buffer serial are never the same twice */
        const float clock = (float)(depth + 1);
        s.n.rg.origin[0] = s.o.rg.origin[0] = s.mirror.rg.origin[0] = clock;
        s.n.rg.up[2] = s.o.rg.up[2] = s.mirror.rg.up[2] = -clock;
        s.n.eye[1] = s.o.eye[1] = s.mirror.eye[1] = 0.5f * clock;
        s.n.gbuf.serial = s.o.gbuf.serial = s.mirror.gbuf.serial = (uint64_t)(depth + 1);
        const old_ctx& b = from.o;
        const bool update = e >= EV_UPDATE_0_1 && b.has_scene && b.n_tris == 4 && b.d_tv_prev != nullptr;
        if (update)
        {
            const bool rebase = (b.motion && b.res_dirty) || (b.dn_motion && b.dt_dirty), nonempty = b.mv_hi > b.mv_lo;
            ++g_count[rebase ? (nonempty ? C_REBASE_NONEMPTY : C_REBASE_EMPTY) : (nonempty ? C_GROW_NONEMPTY : C_GROW_FROM_EMPTY)];
        }
        if (b.d_tv_prev && b.mv_hi > b.mv_lo && ((e == EV_RES_ON && !b.motion && b.dn_motion) || (e == EV_DN_ON && !b.dn_motion && b.motion))) ++g_count[C_ON_WHILE_SHARED];
        if ((e == EV_RES_OFF && b.motion && !b.dn_motion) || (e == EV_DN_OFF && b.dn_motion && !b.motion)) ++g_count[C_LAST_OFF];

        Dev d_new, d_old, d_mir;
        g_dev = &d_new; const int rn = new_apply(&s.n, e);
        g_dev = &d_old; const int ro = old_apply(&s.o, e);
        g_dev = &d_mir; if (mirrored(e) >= 0) old_apply(&s.mirror, mirrored(e));
        ++g_count[C_NODES];
        if (d_new.n > 15 || d_old.n > 15) ++g_count[C_LOG_OVERFLOW];
        bool ok = rn == ro && same(s.n, s.o) && d_new.n == d_old.n && memcmp(d_new.op, d_old.op, sizeof(d_new.op)) == 0;
        for (int p = 0; p < 5; ++p)
        {
            const bool f = old_history_motion(&s.o, p);
            if (f != new_history_motion(&s.n, p)) ok = false;
            if (f) ++g_count[C_FOLLOWED_RES];
            if (s.o.rec_rg_has[p] && s.o.motion && s.o.d_tv_prev && !f)
            {
                if (s.o.rec_gen[p] + 1 == s.o.tvp_gen) ++g_count[C_TAG_OLDER];
                if (s.o.rec_gen[p] == s.o.geo_gen) ++g_count[C_TAG_CURRENT];
            }
        }
        {
            const bool f = old_dn_followed(&s.o);
            if (f != new_dn_followed(&s.n)) ok = false;
            if (f) ++g_count[C_FOLLOWED_DN];
            if (s.o.dt_valid && s.o.dn_motion && s.o.d_tv_prev && !f)
            {
                if (s.o.dt_gen + 1 == s.o.tvp_gen) ++g_count[C_TAG_OLDER];
                if (s.o.dt_gen == s.o.geo_gen) ++g_count[C_TAG_CURRENT];
            }
        }
        if (!ok) ++g_count[C_DIFFER];
        /* the same events with the consumers exchanged leave other kept vertices: the dirty bits are not symmetric */
        if (s.o.d_tv_prev && s.mirror.d_tv_prev && (s.o.tvp_gen != s.mirror.tvp_gen || s.o.mv_lo != s.mirror.mv_lo || s.o.mv_hi != s.mirror.mv_hi)) ++g_count[C_ASYMMETRY];
        if (depth + 1 < DEPTH) step(s, depth + 1);
    }
}
extern "C" void walk(long long* out)
{
    memset(g_count, 0, sizeof(g_count));
    g_bad_copy = 0;
    State start;
    if (!same(start.n, start.o)) ++g_count[C_DIFFER];
    step(start, 0);
    g_count[C_BAD_COPY] = g_bad_copy;
    memcpy(out, g_count, sizeof(g_count));
}

/* ---- the header alone, for the comparison with MotionRef's host rules (a scene always has vertices there) ---- */
static MovedGeometry g_m;
static HistoryTag g_dt;
static bool g_dt_valid;
static const float g_eye0[3] = {0.0f, 0.0f, 0.0f};
extern "C" int hp_scene_set() { g_dt_valid = false; return g_m.scene_set(true) ? 1 : 0; }
extern "C" void hp_new() { g_m = MovedGeometry(); g_dt = HistoryTag(); hp_scene_set(); }
extern "C" int hp_toggle(int consumer, int on) { return (int)g_m.toggle((Consumer)consumer, on != 0, true); }
extern "C" void hp_tagged_reservoir() { g_m.tagged(FOLLOW_RESTIR); }
extern "C" int hp_denoiser_call()
{
    const bool f = g_m.follows(FOLLOW_DENOISER, g_dt, g_dt_valid);
    g_dt.write(rt_raygen{}, g_m.geo_gen, g_eye0, 0);
    g_m.tagged(FOLLOW_DENOISER);
    g_dt_valid = true;
    return f ? 1 : 0;
}
extern "C" void hp_denoiser_reset() { g_dt_valid = false; }
extern "C" int hp_update(uint32_t first, uint32_t count, uint32_t* lo, uint32_t* hi)
{
    const MovedUpdate u = g_m.update(first, count);
    *lo = u.lo; *hi = u.hi;
    return (int)u.kind;
}
/* {geo_gen, kept_gen, lo, hi, kept, toggles, dirty bits} */
extern "C" void hp_state(uint64_t* out)
{
    out[0] = g_m.geo_gen; out[1] = g_m.kept_gen; out[2] = g_m.lo; out[3] = g_m.hi; out[4] = g_m.kept;
    out[5] = g_m.on[FOLLOW_RESTIR]; out[6] = g_m.on[FOLLOW_DENOISER]; out[7] = g_m.dirty[FOLLOW_RESTIR]; out[8] = g_m.dirty[FOLLOW_DENOISER];
}

int main()
{
    static const char* const NAME[N_COUNTS] = {"nodes", "differ", "rebase_nonempty", "rebase_empty", "grow_from_empty", "grow_nonempty", "on_while_shared",
                                               "last_off", "tag_older", "tag_current", "followed_res", "followed_dn", "asymmetry", "bad_copy", "log_overflow"};
    long long out[N_COUNTS];
    walk(out);
    bool ok = out[C_DIFFER] == 0 && out[C_BAD_COPY] == 0 && out[C_LOG_OVERFLOW] == 0;
    for (int k = 0; k < N_COUNTS; ++k)
    {
        printf("%s %lld\n", NAME[k], out[k]);
        if (k != C_DIFFER && k != C_BAD_COPY && k != C_LOG_OVERFLOW && out[k] == 0) ok = false;
    }
    return ok ? 0 : 1;
}
"""

COUNTS = ("nodes", "differ", "rebase_nonempty", "rebase_empty", "grow_from_empty", "grow_nonempty", "on_while_shared", "last_off", "tag_older",
          "tag_current", "followed_res", "followed_dn", "asymmetry", "bad_copy", "log_overflow")
N_EVENTS = 16

_lib = None
_result = None


def write_program(path):
    with open(path, "w") as f:
        f.write(PROGRAM)


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="history_provenance_")
        src, so = os.path.join(d, "history_provenance.cpp"), os.path.join(d, "history_provenance.so")
        write_program(src)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-DDEPTH={DEPTH}", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        _lib = C.CDLL(so)
        _lib.hp_update.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return _lib


def walk():
    global _result
    if _result is None:
        out = (C.c_longlong * len(COUNTS))()
        lib().walk(out)
        _result = dict(zip(COUNTS, out))
        print("history provenance walk:", _result)
    return _result


def test_header_equals_the_restated_statements_after_every_event():
    """the whole state, the device operations with their ranges and the followed-or-not decision of both consumers for every tag"""
    w = walk()
    assert w["differ"] == 0
    assert w["bad_copy"] == 0, "every copy is between the same triangles of the current and the kept vertices, inside the scene"
    assert w["log_overflow"] == 0


def test_the_walk_visited_every_sequence():
    """16 events at every level: a walk that silently visits less does not pass"""
    assert walk()["nodes"] == sum(N_EVENTS ** k for k in range(1, DEPTH + 1))


def test_the_walk_reached_every_situation():
    """each of them at least once, as the restated statements see it: both kinds of re-base and of growth, a toggle going on while the other
    consumer holds the kept vertices with a non-empty range, the last toggle going off, a tag one generation older than the kept
    vertices and one of the current generation (neither followed), a followed tag for each consumer, and the same events with the
    consumers exchanged leaving other kept vertices (res_dirty is set whether its toggle is on or not and survives it, dt_dirty not)"""
    w = walk()
    for k in ("rebase_nonempty", "rebase_empty", "grow_from_empty", "grow_nonempty", "on_while_shared", "last_off", "tag_older", "tag_current",
              "followed_res", "followed_dn", "asymmetry"):
        assert w[k] > 0, k


def _state(L):
    out = (C.c_uint64 * 9)()
    L.hp_state(out)
    return dict(zip(("geo_gen", "kept_gen", "lo", "hi", "kept", "motion", "on", "res_dirty", "dt_dirty"), (int(v) for v in out)))


def _ref_state(M):
    return dict(geo_gen=M.geo_gen, kept_gen=M.tvp_gen, lo=M.lo, hi=M.hi, kept=int(M.tv_prev is not None), motion=int(M.motion), on=int(M.on),
                res_dirty=int(M.res_dirty), dt_dirty=int(M.dt_dirty))


def test_header_beside_the_python_model_of_the_gpu_tests():
    """MotionRef's host rules (set_scene, toggle, toggle_motion, frame, update, range; a 1 x 1 call of a pixel that hit nothing for
    the denoiser's tag) and the header, event by event: equal generations, ranges, kept-or-not, toggles and dirty bits, the same copy
    asked of an update, the same followed-or-not for the denoiser's call"""
    import denoise_motion_ref as dm

    L = lib()
    tris = np.zeros((4, 15), np.float32)
    tris[:, 0:9] = np.arange(36, dtype=np.float32).reshape(4, 9)
    vis = np.array([[0, 0, -1, 0]], np.int32).view(np.float32)
    rg, eye, acc = np.arange(9, dtype=np.float32), np.zeros(3, np.float32), np.zeros((1, 4), np.float32)
    spans = ((0, 1), (1, 2), (3, 1), (0, 4))
    seen = dict(followed=0, rebase=0, grow=0, events=0)
    for seed in range(40):
        rng = np.random.default_rng(seed)
        M = dm.MotionRef(1, 1, tris, iterations=0)
        L.hp_new()
        assert _state(L) == _ref_state(M)
        for _ in range(60):
            e = int(rng.integers(0, 10))
            if e == 0:
                M.set_scene(tris)
                assert L.hp_scene_set() == int(M.tv_prev is not None)
            elif e in (1, 2):
                M.toggle(e == 1)
                L.hp_toggle(1, int(e == 1))
            elif e in (3, 4):
                M.toggle_motion(e == 3)
                L.hp_toggle(0, int(e == 3))
            elif e == 5:
                M.frame()
                L.hp_tagged_reservoir()
            elif e == 6:
                M(vis, eye, rg, acc)
                assert bool(L.hp_denoiser_call()) == M.followed
                seen["followed"] += M.followed
            elif e == 7 and rng.integers(0, 4) == 0:
                M.reset()
                L.hp_denoiser_reset()
            elif e >= 8:
                first, count = spans[int(rng.integers(0, 4))]
                before = _ref_state(M)
                kept_before = None if M.tv_prev is None else M.tv_prev.copy()
                M.update(np.full((count, 15), float(M.geo_gen + 1), np.float32), first)
                lo, hi = C.c_uint32(), C.c_uint32()
                kind = L.hp_update(first, count, C.byref(lo), C.byref(hi))
                assert (kind != 0) == bool(before["kept"])
                if kind == 1:  # re-base: the model copied exactly the old range
                    assert (lo.value, hi.value) == (before["lo"], before["hi"]) and M.tvp_gen == before["geo_gen"]
                    changed = np.flatnonzero((kept_before != M.tv_prev).reshape(4, 60).any(axis=1))
                    assert all(lo.value <= t < hi.value for t in changed)
                    seen["rebase"] += 1
                elif kind == 2:
                    assert np.array_equal(kept_before, M.tv_prev)
                    seen["grow"] += 1
            assert _state(L) == _ref_state(M)
            assert M.range() == dict(lo=_state(L)["lo"], hi=_state(L)["hi"], generation=_state(L)["kept_gen"])
            seen["events"] += 1
    print("header beside MotionRef:", seen)
    assert seen["followed"] > 0 and seen["rebase"] > 0 and seen["grow"] > 0
