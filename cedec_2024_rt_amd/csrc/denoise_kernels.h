/*
 * denoise_kernels.h — the gfx950 kernels of rt_denoise (included once, by restir_rt.hip, after frame_kernels.h).
 *
 * Whole-frame contexts only (lrow0 = 0): buffer index = row * W + x. All arithmetic is denoise_math.h's; the loops below are
 * what tests/denoise_ref.py restates on the CPU (tap order dy outer, dx inner).
 *
 *   k_denoise_guide   one primary ray per pixel (k_raycast's ray and closest-hit walk, tile order of rt_tuning key 0):
 *                     gx = {x_p, f_p}, gn = {n_p, guide word}, and the rt_visibility record of the hit
 *   k_denoise_demod   col = {e, 0} for participating pixels, {0, 0, 0, -1} for the others
 *   k_denoise_var     col' = {e, var}: moments over the (2R+1)^2 window at step 1
 *   k_denoise_iter    one a-trous level at step s (rt_tuning key 28 = 0: per-lane gathers, tiles in XCD bands as the spatial pass)
 *   k_denoise_iter_lds the same level over 16 x 16 blocks of one residue lattice {p = r mod s} staged in LDS with a 2-point apron
 *                     (key 28 = 1: 20 x 20 records of 48 B whatever the step)
 *   FINAL forms of the level (and k_denoise_output for 0 iterations): HDR value + RGBA8 (tone_map_rgba8)
 *
 * rt_denoise_temporal puts two kernels in place of demodulation and variance and reuses the others:
 *   k_denoise_temporal  reprojection into the previous camera, demodulation and integration: col = {c, 0} (or {0, 0, 0, -1}) and
 *                       the moments record {mu1, mu2, h, 0}
 *   k_denoise_var_hist  col' = {c, var}: the temporal variance where h >= 4, k_denoise_var's window elsewhere
 *   k_denoise_temporal_motion  k_denoise_temporal for a followed call of rt_denoise_temporal_motion (denoise_motion.h): pixels on a
 *                       triangle rt_scene_update moved look their history up from where their surface point was
 *
 * An adapted call of rt_denoise_temporal_antilag (denoise_antilag.h) puts two kernels in place of k_denoise_temporal{,_motion}:
 *   k_denoise_antilag_gather<MOTION>  dn_temporal_pixel up to the blend: {e, l_h} -> d_dn_col[0] (free until k_denoise_var_hist),
 *                       {c_prev, 0} -> d_dn_col[1], {mu1_prev, mu2_prev, h_prev, 0} -> the current moments
 *   k_denoise_antilag   32 x 8 pixels per workgroup; {n, l_h} and l_e of the tile and a halo of `radius` in LDS; lambda', the blend,
 *                       colour and moments in place at the pixel itself
 */
#pragma once
#include "denoise_math.h"
#include "denoise_motion.h"
#include "denoise_antilag.h"

/* rt_tuning key 28 default: the residue lattice in LDS (1), 1.13 against 1.19 ms of filter at 5 iterations, 1080p */
#ifndef DN_LAYOUT_DEFAULT
#define DN_LAYOUT_DEFAULT 1
#endif

struct DnParams
{
    int iterations;
    float sigma_l, sigma_x;
    int normal_power_log2, variance_radius;
};

/* ------------------------------------------------------------------ guide */
template <bool WS>
__global__ __launch_bounds__(TRACE_BLOCK, WS ? RT_RAYCAST_WS_WAVES : RT_RAYCAST_WAVES) void k_denoise_guide(SceneView S, FrameParams P, float4* __restrict__ vis,
                                                                                                         float4* __restrict__ gx, float4* __restrict__ gn)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_stack[(WS ? WIDE_LDS_ROWS_CLOSEST : WIDE_LDS_STACK) * TRACE_BLOCK];
    int x, row;
    if (!tile_pixel<TRACE_BLOCK>(P, x, row)) return;
    const int yi = P.H - 1 - row;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const f3 rd = primary_direction(P, x, yi);
    Hit h;
    h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.prim = -1;
    if (WS) closest_ws<TRACE_BLOCK>(S.wide, S.bvh.tv, s_stack, P.rg_origin, rd, 0.0f, kFltMax, h);
    else trace_wide<false, false, TRACE_BLOCK>(S.wide, s_stack, P.rg_origin, rd, 0.0f, kFltMax, h, nullptr, RT_BARY_TV(S));
    vis[li] = make_float4(h.u, h.v, as_float(h.prim), as_float(0));
    if (h.prim < 0)
    {
        gx[li] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        gn[li] = make_float4(0.0f, 0.0f, 0.0f, as_float(dn_guide_word(-1, false)));
        return;
    }
    f3 v0, v1, v2, p, n;
    load_tri(S.bvh.tv, h.prim, v0, v1, v2);
    dn_surface(v0, v1, v2, h.u, h.v, P.eye, p, n);
    const bool emissive = as_uint(S.trimat[2 * (size_t)h.prim].w) != 0u;
    gx[li] = make_float4(p.x, p.y, p.z, dn_pixel_size(p, P.eye, P.rg_up, P.H));
    gn[li] = make_float4(n.x, n.y, n.z, as_float(dn_guide_word(h.prim, emissive)));
}

RT_DEV f3 dn_albedo(const float4* __restrict__ trimat, uint32_t word)
{
    const float4 k = trimat[2 * (size_t)dn_tri(word)];
    return F3(k.x, k.y, k.z);
}

/* ------------------------------------------------------------------ prep */
__global__ __launch_bounds__(BLOCK) void k_denoise_demod(FrameParams P, const float4* __restrict__ trimat, const float4* __restrict__ accum,
                                                         const float4* __restrict__ gn, float4* __restrict__ col)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const uint32_t word = as_uint(gn[li].w);
    const float4 A = accum[li];
    if (dn_kind(word) != DN_KIND_SURFACE || A.w == 0.0f)
    {
        col[li] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    const f3 e = dn_demodulate(A, dn_albedo(trimat, word));
    col[li] = make_float4(e.x, e.y, e.z, 0.0f);
}

/* the luminance variance of participating pixel (x, row) over the (2R+1)^2 window at step 1 */
RT_DEV float dn_window_variance(const FrameParams& P, const DnParams& D, int x, int row, size_t li, const float4* __restrict__ gx,
                                const float4* __restrict__ gn, const float4* __restrict__ cin)
{
    const float4 xp4 = gx[li], np4 = gn[li];
    const f3 xp = F3(xp4.x, xp4.y, xp4.z), np = F3(np4.x, np4.y, np4.z);
    const int R = D.variance_radius;
    DnMoments m = dn_moments_init();
    for (int dy = -R; dy <= R; ++dy)
    {
        const int qr = row + dy;
        if (qr < 0 || qr >= P.H) continue;
        for (int dx = -R; dx <= R; ++dx)
        {
            const int qx = x + dx;
            if (qx < 0 || qx >= P.W) continue;
            const size_t qi = (size_t)qx + (size_t)qr * P.W;
            const float4 cq = cin[qi];
            if (cq.w < 0.0f) continue;
            const float4 xq4 = gx[qi], nq4 = gn[qi];
            const float wn = dn_normal_weight(np, F3(nq4.x, nq4.y, nq4.z), D.normal_power_log2);
            const float dxp = dn_plane_distance(np, xp, F3(xq4.x, xq4.y, xq4.z), D.sigma_x, 1.0f, xp4.w);
            dn_moments_add(m, dn_variance_weight(wn, dxp), dn_luminance(cq));
        }
    }
    return dn_moments_variance(m);
}
__global__ __launch_bounds__(BLOCK) void k_denoise_var(FrameParams P, DnParams D, const float4* __restrict__ gx, const float4* __restrict__ gn,
                                                       const float4* __restrict__ cin, float4* __restrict__ cout)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const float4 cp = cin[li];
    if (cp.w < 0.0f)
    {
        cout[li] = cp;
        return;
    }
    cout[li] = make_float4(cp.x, cp.y, cp.z, dn_window_variance(P, D, x, row, li, gx, gn, cin));
}

/* ------------------------------------------------------------------ temporal prep (rt_denoise_temporal) */
struct DnTemporal
{
    f3 rg_origin, rg_right, rg_up; /* the previous call's RayGenerator */
    float alpha_c, alpha_m;
    int has_history; /* 0: the first call after a reset (the previous buffers are not read) */
};
/* what a followed call adds (rt_denoise_temporal_motion, denoise_motion.h): read by k_denoise_temporal_motion only */
struct DnMotion
{
    f3 eye_prev;                       /* the eye of the previous call */
    uint32_t lo, hi;                   /* the moved range */
    const float4* __restrict__ tv_prev; /* the vertices of the history's generation (layout of the BVH's tv: 3 records per triangle) */
    const float4* __restrict__ vis;     /* this call's guide hits {u, v, prim, 0} */
};
/* one pass per pixel: 2 guide records, the accumulation, the albedo, and per valid tap 4 records of the previous frame.
 * MOTION (a followed call): + the pixel's vis record, and for the lanes on a triangle of the moved range the 48 bytes of its previous
 * vertices; reprojection and tap test then run on the previous surface point and normal. MOTION = false is the r10 kernel.
 * GATHER (an adapted call of rt_denoise_temporal_antilag): everything up to the blend; k_denoise_antilag finishes the pixel. */
template <bool MOTION, bool GATHER = false>
RT_DEV void dn_temporal_pixel(const FrameParams& P, const DnTemporal& T, const DnMotion* M, const float4* __restrict__ trimat,
                              const float4* __restrict__ accum, const float4* __restrict__ gx, const float4* __restrict__ gn,
                              const float4* __restrict__ pgx, const float4* __restrict__ pgn, const float4* __restrict__ hcol,
                              const float4* __restrict__ hmom, float4* __restrict__ col, float4* __restrict__ mom,
                              float4* __restrict__ ecol = nullptr)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const float4 np4 = gn[li];
    const uint32_t word = as_uint(np4.w);
    const float4 A = accum[li];
    if (dn_kind(word) != DN_KIND_SURFACE || A.w == 0.0f)
    {
        if (GATHER) ecol[li] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        col[li] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        mom[li] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const f3 e = dn_demodulate(A, dn_albedo(trimat, word));
    const float4 xp4 = gx[li];
    f3 xp = F3(xp4.x, xp4.y, xp4.z), np = F3(np4.x, np4.y, np4.z); /* the lookup point and normal (x_l, n_l) */
    if (MOTION)
    {
        const float4 vq = M->vis[li];
        const int prim = dn_tri(word);
        if (tm_in_range(prim, M->lo, M->hi))
        {
            f3 v0, v1, v2;
            load_tri(M->tv_prev, prim, v0, v1, v2);
            dn_motion_lookup(v0, v1, v2, vq.x, vq.y, M->eye_prev, xp, np);
        }
    }
    DnHistory s = dn_history_init();
    float px, pr;
    if (T.has_history && dn_reproject(xp, T.rg_origin, T.rg_right, T.rg_up, P.W, P.H, px, pr))
    {
        int x0, r0;
        float w[4];
        dn_bilinear(px, pr, x0, r0, w);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const int qx = x0 + (k & 1), qr = r0 + (k >> 1);
            if (qx < 0 || qx >= P.W || qr < 0 || qr >= P.H) continue;
            const size_t qi = (size_t)qx + (size_t)qr * P.W;
            const float4 mq = hmom[qi], nq4 = pgn[qi], xq4 = pgx[qi];
            if (!dn_temporal_tap_valid(np, xp, xp4.w, as_uint(nq4.w), mq.z, F3(nq4.x, nq4.y, nq4.z), F3(xq4.x, xq4.y, xq4.z))) continue;
            dn_history_add(s, w[k], hcol[qi], mq);
        }
    }
    if (GATHER)
    {
        /* the quotients of dn_temporal_integrate, kept for dn_antilag_integrate; l_h = -1: no history */
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float lh = -1.0f;
        if (s.sw >= DN_TEMPORAL_WEIGHT_MIN)
        {
            c = make_float4(s.r / s.sw, s.g / s.sw, s.b / s.sw, 0.0f);
            m = make_float4(s.m1 / s.sw, s.m2 / s.sw, s.h, 0.0f);
            lh = dn_luminance(c);
        }
        ecol[li] = make_float4(e.x, e.y, e.z, lh);
        col[li] = c;
        mom[li] = m;
        return;
    }
    float4 c, m;
    dn_temporal_integrate(s, e, T.alpha_c, T.alpha_m, c, m);
    col[li] = c;
    mom[li] = m;
}
__global__ __launch_bounds__(BLOCK) void k_denoise_temporal(FrameParams P, DnTemporal T, const float4* __restrict__ trimat,
                                                            const float4* __restrict__ accum, const float4* __restrict__ gx,
                                                            const float4* __restrict__ gn, const float4* __restrict__ pgx,
                                                            const float4* __restrict__ pgn, const float4* __restrict__ hcol,
                                                            const float4* __restrict__ hmom, float4* __restrict__ col, float4* __restrict__ mom)
{
    dn_temporal_pixel<false>(P, T, nullptr, trimat, accum, gx, gn, pgx, pgn, hcol, hmom, col, mom);
}
__global__ __launch_bounds__(BLOCK) void k_denoise_temporal_motion(FrameParams P, DnTemporal T, DnMotion M, const float4* __restrict__ trimat,
                                                                   const float4* __restrict__ accum, const float4* __restrict__ gx,
                                                                   const float4* __restrict__ gn, const float4* __restrict__ pgx,
                                                                   const float4* __restrict__ pgn, const float4* __restrict__ hcol,
                                                                   const float4* __restrict__ hmom, float4* __restrict__ col, float4* __restrict__ mom)
{
    dn_temporal_pixel<true>(P, T, &M, trimat, accum, gx, gn, pgx, pgn, hcol, hmom, col, mom);
}
/* ---- rt_denoise_temporal_antilag: the two kernels of an adapted call ---- */
template <bool MOTION>
__global__ __launch_bounds__(BLOCK) void k_denoise_antilag_gather(FrameParams P, DnTemporal T, DnMotion M, const float4* __restrict__ trimat,
                                                                  const float4* __restrict__ accum, const float4* __restrict__ gx,
                                                                  const float4* __restrict__ gn, const float4* __restrict__ pgx,
                                                                  const float4* __restrict__ pgn, const float4* __restrict__ hcol,
                                                                  const float4* __restrict__ hmom, float4* __restrict__ ecol,
                                                                  float4* __restrict__ col, float4* __restrict__ mom)
{
    dn_temporal_pixel<MOTION, true>(P, T, &M, trimat, accum, gx, gn, pgx, pgn, hcol, hmom, col, mom, ecol);
}
/* Workgroup b = tile (b % ntx, b / ntx) of DN_AL_TILE_W x DN_AL_TILE_H pixels, one per lane. LDS: per entry of the tile and its halo
 * of `radius` {n, l_h} (16 B) and l_e (4 B), l_h = -1 outside the image: (32 + 8) x (8 + 8) entries at radius 4 = 12 800 B. ecol =
 * {e, l_h}, col = {c_prev, 0} / {0, 0, 0, -1} and mom = {mu1_prev, mu2_prev, h_prev, 0} as k_denoise_antilag_gather left them; col
 * and mom are rewritten at the lane's own pixel only, which no other lane reads. The tile: 32 x 8 measured 0.071 ms at 1920 x 1080
 * and radius 4 against 0.077 for 16 x 16 and 0.074 for 32 x 16; two or four pixels of a column per lane, which read each LDS entry
 * once for all of them, measured slower (0.082 to 0.128: docs/MEASUREMENT_LOG_r30.md). */
constexpr int DN_AL_TILE_W = 32, DN_AL_TILE_H = 8, DN_AL_THREADS = DN_AL_TILE_W * DN_AL_TILE_H;
constexpr int DN_AL_ENTRIES = (DN_AL_TILE_W + 2 * DN_ANTILAG_RADIUS_MAX) * (DN_AL_TILE_H + 2 * DN_ANTILAG_RADIUS_MAX);
__global__ __launch_bounds__(DN_AL_THREADS) void k_denoise_antilag(int W, int H, int ntx, DnAntilag L, float alpha_c, float alpha_m,
                                                                   const float4* __restrict__ gn, const float4* __restrict__ ecol,
                                                                   float4* __restrict__ col, float4* __restrict__ mom)
{
    __shared__ float4 s_n[DN_AL_ENTRIES];
    __shared__ float s_le[DN_AL_ENTRIES];
    const int R = L.radius, A = DN_AL_TILE_W + 2 * R, N = A * (DN_AL_TILE_H + 2 * R);
    const int by = (int)blockIdx.x / ntx, bx = (int)blockIdx.x - by * ntx;
    const int x0 = bx * DN_AL_TILE_W - R, r0 = by * DN_AL_TILE_H - R; /* pixel of apron entry (0, 0) */
    for (int k = (int)threadIdx.x; k < N; k += DN_AL_THREADS)
    {
        const int jj = k / A, ii = k - jj * A;
        const int qx = x0 + ii, qr = r0 + jj;
        float4 nq = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        float le = 0.0f;
        if (qx >= 0 && qx < W && qr >= 0 && qr < H)
        {
            const size_t qi = (size_t)qx + (size_t)qr * W;
            const float4 eq = ecol[qi], g = gn[qi];
            nq = make_float4(g.x, g.y, g.z, eq.w);
            le = dn_luminance(eq);
        }
        s_n[k] = nq;
        s_le[k] = le;
    }
    __syncthreads();
    const int ti = (int)threadIdx.x % DN_AL_TILE_W, tj = (int)threadIdx.x / DN_AL_TILE_W;
    const int x = x0 + R + ti, row = r0 + R + tj;
    if (x >= W || row >= H) return;
    const int c0 = (tj + R) * A + (ti + R);
    const float4 np4 = s_n[c0];
    const f3 np = F3(np4.x, np4.y, np4.z);
    const bool window = dn_antilag_has_history(np4.w); /* l_h = -1 also where the pixel does not participate */
    DnGradient g = dn_gradient_init();
    if (window)
        for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx)
            {
                const int k = c0 + dy * A + dx;
                const float4 nq = s_n[k];
                const float le = s_le[k]; /* read with nq, not behind the test: both LDS reads are in flight together */
                if (dn_antilag_member(np, F3(nq.x, nq.y, nq.z), nq.w)) dn_gradient_add(g, le, nq.w);
            }
    const size_t li = (size_t)x + (size_t)row * W;
    const float4 cprev = col[li];
    if (cprev.w < 0.0f) return; /* does not participate: {0, 0, 0, -1} and zero moments are in place */
    const float4 ep = ecol[li];
    const f3 e = F3(ep.x, ep.y, ep.z);
    float4 c, m;
    if (!window) dn_antilag_first(e, c, m);
    else dn_antilag_integrate(cprev, mom[li], e, alpha_c, alpha_m, dn_antilag_response(dn_gradient_lambda(g, L.floor), L.lo, L.hi), c, m);
    col[li] = c;
    mom[li] = m;
}
__global__ __launch_bounds__(BLOCK) void k_denoise_var_hist(FrameParams P, DnParams D, const float4* __restrict__ gx, const float4* __restrict__ gn,
                                                            const float4* __restrict__ mom, const float4* __restrict__ cin, float4* __restrict__ cout)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const float4 cp = cin[li];
    if (cp.w < 0.0f)
    {
        cout[li] = cp;
        return;
    }
    const float4 m = mom[li];
    const float var = m.z >= DN_HISTORY_VARIANCE_MIN ? dn_temporal_variance(m) : dn_window_variance(P, D, x, row, li, gx, gn, cin);
    cout[li] = make_float4(cp.x, cp.y, cp.z, var);
}

/* ------------------------------------------------------------------ one a-trous level */
/* TAP(dx, dy, cq, xq, nq) loads tap (dx, dy) of the 5 x 5 at the level's step and returns false if it is outside the image or
 * does not participate; p = TAP(0, 0) participates (the caller checked) */
template <typename Tap>
RT_DEV float4 dn_level(const DnParams& D, float step, const float4& cp, const float4& xp4, const float4& np4, Tap tap)
{
    const f3 xp = F3(xp4.x, xp4.y, xp4.z), np = F3(np4.x, np4.y, np4.z);
    DnPrefilter g = dn_prefilter_init();
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
        {
            float4 cq, xq, nq;
            if (tap(dx, dy, cq, xq, nq)) dn_prefilter_add(g, dn_k1(dx) * dn_k1(dy), cq.w);
        }
    const float gvar = dn_prefilter_result(g);
    const float lp = dn_luminance(cp);
    DnFilter f = dn_filter_init();
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx)
        {
            float4 cq, xq, nq;
            if (!tap(dx, dy, cq, xq, nq)) continue;
            const float h = dn_h1(dx) * dn_h1(dy);
            const float wn = dn_normal_weight(np, F3(nq.x, nq.y, nq.z), D.normal_power_log2);
            const float dl = dn_luminance_distance(lp, dn_luminance(cq), D.sigma_l, gvar);
            const float dxp = dn_plane_distance(np, xp, F3(xq.x, xq.y, xq.z), D.sigma_x, step, xp4.w);
            dn_filter_add(f, dn_tap_weight(h, wn, dl, dxp), cq);
        }
    return dn_filter_result(f);
}
/* a non-participating pixel's output: its accumulation value as it is */
template <bool FINAL>
RT_DEV void dn_store(size_t li, const float4& out, bool part, uint32_t word, const float4* __restrict__ trimat, const float4* __restrict__ accum,
                     float4* __restrict__ cout, float4* __restrict__ hdr, uint32_t* __restrict__ pixels)
{
    if (!FINAL || cout) cout[li] = out; /* FINAL with cout: the level that also feeds rt_denoise_temporal's history (1 iteration) */
    if (!FINAL) return;
    float4 v;
    if (part)
    {
        const float4 r = dn_remodulate(out, dn_albedo(trimat, word));
        v = make_float4(r.x, r.y, r.z, r.w);
    }
    else v = accum[li];
    hdr[li] = v;
    pixels[li] = tone_map_rgba8(v);
}

template <bool FINAL>
__global__ __launch_bounds__(BLOCK) void k_denoise_iter(FrameParams P, DnParams D, int step, const float4* __restrict__ trimat,
                                                        const float4* __restrict__ accum, const float4* __restrict__ gx, const float4* __restrict__ gn,
                                                        const float4* __restrict__ cin, float4* __restrict__ cout, float4* __restrict__ hdr,
                                                        uint32_t* __restrict__ pixels)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const float4 cp = cin[li];
    const float4 np4 = gn[li];
    const bool part = cp.w >= 0.0f;
    float4 out = cp;
    if (part)
    {
        const int W = P.W, H = P.H;
        auto tap = [&](int dx, int dy, float4& cq, float4& xq, float4& nq) -> bool {
            const int qx = x + dx * step, qr = row + dy * step;
            if (qx < 0 || qx >= W || qr < 0 || qr >= H) return false;
            const size_t qi = (size_t)qx + (size_t)qr * W;
            cq = cin[qi];
            if (cq.w < 0.0f) return false;
            xq = gx[qi];
            nq = gn[qi];
            return true;
        };
        out = dn_level(D, (float)step, cp, gx[li], np4, tap);
    }
    dn_store<FINAL>(li, out, part, as_uint(np4.w), trimat, accum, cout, hdr, pixels);
}

/* key 28 = 1. Workgroup b: residue r = (rx, ry) of the step's lattice, block (bx, by) of 16 x 16 lattice points; lattice point
 * (i, j) of residue r = pixel (rx + s i, ry + s j). Every tap of a lattice point is a lattice point of the same residue, so a
 * 20 x 20 apron of the lattice holds all of them (and the 3 x 3 of the prefilter) for any step. */
constexpr int DN_LDS_BLOCK = 16, DN_LDS_APRON = DN_LDS_BLOCK + 4;
template <bool FINAL>
__global__ __launch_bounds__(DN_LDS_BLOCK * DN_LDS_BLOCK) void k_denoise_iter_lds(FrameParams P, DnParams D, int step, int nbx, int nby,
                                                        const float4* __restrict__ trimat, const float4* __restrict__ accum,
                                                        const float4* __restrict__ gx, const float4* __restrict__ gn,
                                                        const float4* __restrict__ cin, float4* __restrict__ cout, float4* __restrict__ hdr,
                                                        uint32_t* __restrict__ pixels)
{
    constexpr int A = DN_LDS_APRON, N = A * A;
    __shared__ float4 s_c[N], s_x[N], s_n[N];
    const int b = (int)blockIdx.x, per_res = nbx * nby;
    const int res = b / per_res, rem = b - res * per_res;
    const int ry = res / step, rx = res - ry * step;
    const int by = rem / nbx, bx = rem - by * nbx;
    const int i0 = bx * DN_LDS_BLOCK - 2, j0 = by * DN_LDS_BLOCK - 2; /* lattice coordinates of apron entry (0, 0) */
    const int W = P.W, H = P.H;
    for (int k = (int)threadIdx.x; k < N; k += DN_LDS_BLOCK * DN_LDS_BLOCK)
    {
        const int jj = k / A, ii = k - jj * A;
        const int qx = rx + step * (i0 + ii), qr = ry + step * (j0 + jj);
        if (qx >= 0 && qx < W && qr >= 0 && qr < H)
        {
            const size_t qi = (size_t)qx + (size_t)qr * W;
            s_c[k] = cin[qi];
            s_x[k] = gx[qi];
            s_n[k] = gn[qi];
        }
        else s_c[k] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    }
    __syncthreads();
    const int ti = (int)threadIdx.x % DN_LDS_BLOCK, tj = (int)threadIdx.x / DN_LDS_BLOCK;
    const int x = rx + step * (i0 + 2 + ti), row = ry + step * (j0 + 2 + tj);
    if (x >= W || row >= H) return;
    const size_t li = (size_t)x + (size_t)row * W;
    const int c0 = (tj + 2) * A + (ti + 2);
    const float4 cp = s_c[c0];
    const float4 np4 = s_n[c0];
    const bool part = cp.w >= 0.0f;
    float4 out = cp;
    if (part)
    {
        auto tap = [&](int dx, int dy, float4& cq, float4& xq, float4& nq) -> bool {
            const int k = c0 + dy * A + dx;
            cq = s_c[k];
            if (cq.w < 0.0f) return false;
            xq = s_x[k];
            nq = s_n[k];
            return true;
        };
        out = dn_level(D, (float)step, cp, s_x[c0], np4, tap);
    }
    dn_store<FINAL>(li, out, part, as_uint(np4.w), trimat, accum, cout, hdr, pixels);
}

/* 0 iterations: the demodulated value remodulated as it is */
__global__ __launch_bounds__(BLOCK) void k_denoise_output(FrameParams P, const float4* __restrict__ trimat, const float4* __restrict__ accum,
                                                          const float4* __restrict__ gn, const float4* __restrict__ col, float4* __restrict__ hdr,
                                                          uint32_t* __restrict__ pixels)
{
    int x, row;
    if (!tile_pixel(P, x, row)) return;
    const size_t li = (size_t)x + (size_t)row * P.W;
    const float4 cp = col[li];
    dn_store<true>(li, cp, cp.w >= 0.0f, as_uint(gn[li].w), trimat, accum, nullptr, hdr, pixels);
}
