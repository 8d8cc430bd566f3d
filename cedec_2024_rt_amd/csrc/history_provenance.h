/* history_provenance.h — under which camera and which geometry a history was written, and which vertices are kept to follow it
 * (rt_temporal_reprojection, rt_temporal_motion, rt_denoise_temporal_motion; DESIGN.md sections 13-15 and 17). Host only, plain C++17,
 * no HIP include of its own: tests/test_history_provenance_cpu.py walks it beside the statements it replaced in restir_rt.hip.
 * Nothing here touches the device: a transition returns what restir_rt.hip has to do there. */
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/restir_rt.h"
#include "denoise_motion.h" /* dn_motion_followed: the followed-or-not expression, shared with tests/denoise_motion_ref.py */

namespace rt
{
/* What a history buffer was written under: the RayGenerator, the geometry generation and the eye (valid under `has`). A reservoir
 * buffer also carries gserial, the serial of the G-buffer its shaded bits belong to (k_refresh_shaded): valid whether `has` or not,
 * and set alone where only the bits were refreshed. A copy of a buffer takes the whole tag: plain assignment.
 * light_gen (rt_temporal_light_motion): the generation up to which the LIGHT side of the records (sample point,
 * normal, radiance) is current. Set with gen by write, advanced alone by an update that re-based the buffer's samples onto the new
 * emitters; gen stays what it was, rt_temporal_motion reads it. */
struct HistoryTag
{
    rt_raygen rg = {};
    bool has = false;
    uint64_t gen = 0;
    float eye[3] = {0.0f, 0.0f, 0.0f};
    uint64_t gserial = 0;
    uint64_t light_gen = 0;
    void write(const rt_raygen& rg_, uint64_t gen_, const float eye_[3], uint64_t gserial_)
    {
        rg = rg_; has = true; gen = gen_; memcpy(eye, eye_, sizeof(eye)); gserial = gserial_; light_gen = gen_;
    }
    /* do the records' light samples describe generation geo_gen, the one an update is about to end? Written under it, or carried
     * to it by the update before: two updates with no frame between them are both followed. An older or untagged buffer is not. */
    bool light_current(uint64_t geo_gen) const { return has && std::max(gen, light_gen) == geo_gen; }
    /* the update that ends generation geo_gen has re-based this buffer's samples (only a light_current buffer is re-based) */
    void light_rebased(uint64_t geo_gen) { light_gen = geo_gen + 1; }
    /* the update that ends generation geo_gen is followed (the toggle is on) and its span held no emissive triangle: a light_current
     * buffer's samples lie on triangles that keep their bytes, so they describe the next generation as they are. Without this a box
     * moved before a lamp, with no frame between the two updates, would end the chain that the other order keeps. */
    void light_untouched(uint64_t geo_gen) { if (light_current(geo_gen)) light_gen = geo_gen + 1; }
};

/* the two consumers of the kept vertices: the ReSTIR history (rt_temporal_motion) and the denoiser's (rt_denoise_temporal_motion) */
enum Consumer { FOLLOW_RESTIR = 0, FOLLOW_DENOISER = 1 };
/* what a toggle asks of the device: nothing; drain the stream (launches in flight may read the kept vertices), free them and keep a
 * copy of all current vertices; drain and free */
enum KeptAction { KEPT_NOTHING, KEPT_DRAIN_FREE_COPY, KEPT_DRAIN_FREE };
/* what an update asks of the device BEFORE the span is written: nothing (no kept vertices); bring the kept vertices to the current
 * ones over the OLD range [lo, hi) (may be empty), a new range then starts at the span; nothing, the range grew to cover the span */
struct MovedUpdate
{
    enum Kind { NONE, REBASE, GROW } kind;
    uint32_t lo, hi;
};

/* The moved range. geo_gen counts updates since scene_set. While a toggle is on and the scene has vertices, the kept vertices
 * (`kept`: they exist) are those of generation kept_gen: equal to the current ones outside [lo, hi), the cover of the spans updated
 * since. dirty[k]: consumer k's history was tagged since the last update, so the next update re-bases the kept vertices to the
 * generation it ends instead of growing the range.
 * The two consumers are NOT symmetric, and this is kept as it was found: dirty[FOLLOW_RESTIR] is set by every tag whether its toggle is
 * on or not and survives a change of that toggle; dirty[FOLLOW_DENOISER] is set only while its toggle is on and is cleared when that
 * toggle changes. So a reservoir buffer tagged before rt_temporal_motion goes on re-bases at the next update; a denoiser history
 * tagged before rt_denoise_temporal_motion goes on does not. */
struct MovedGeometry
{
    uint64_t geo_gen = 0, kept_gen = 0;
    uint32_t lo = 0, hi = 0;
    bool kept = false;
    bool on[2] = {false, false}, dirty[2] = {false, false};

    /* a new scene: generations and range from 0. Returns whether a copy of all its vertices is to be kept (the old ones are gone
     * with the old scene either way) */
    bool scene_set(bool has_vertices)
    {
        geo_gen = 0; dirty[0] = dirty[1] = false;
        return keep_all(has_vertices);
    }
    /* the first toggle going on keeps a copy, the last going off frees it; a toggle that changes while the other consumer holds the
     * kept vertices leaves them and the range alone */
    KeptAction toggle(Consumer k, bool v, bool has_vertices)
    {
        const bool was = on[k];
        on[k] = v;
        if (v == was) return KEPT_NOTHING;
        if (k == FOLLOW_DENOISER) dirty[k] = false; /* a history tagged while the toggle was off, or before this moment, re-bases nothing */
        if (on[1 - k]) return KEPT_NOTHING;
        return keep_all(has_vertices) ? KEPT_DRAIN_FREE_COPY : KEPT_DRAIN_FREE;
    }
    /* consumer k's history (a reservoir buffer / the denoiser's) was written under the current generation */
    void tagged(Consumer k)
    {
        if (k == FOLLOW_RESTIR || on[k]) dirty[k] = true;
    }
    /* triangles [first, first + count) are about to change. A history written since the last update by a consumer whose toggle is on
     * carries the generation this update ends: re-base. Otherwise no history of the generations in between exists: grow. */
    MovedUpdate update(uint32_t first, uint32_t count)
    {
        MovedUpdate u = {MovedUpdate::NONE, lo, hi};
        if (kept)
        {
            if ((on[0] && dirty[0]) || (on[1] && dirty[1])) { u.kind = MovedUpdate::REBASE; kept_gen = geo_gen; lo = first; hi = first + count; }
            else
            {
                u.kind = MovedUpdate::GROW;
                if (hi > lo) { lo = std::min(lo, first); hi = std::max(hi, first + count); }
                else { lo = first; hi = first + count; }
            }
        }
        ++geo_gen;
        dirty[0] = dirty[1] = false;
        return u;
    }
    /* does a launch that reads the history under `tag` follow the moved triangles? A history of exactly the generation the kept
     * vertices describe, which is not the current one; an older one, or one of the current generation, gets the cameras only.
     * valid: what else the caller knows of the history's existence (the denoiser's dt_valid). */
    bool follows(Consumer k, const HistoryTag& tag, bool valid = true) const
    {
        return dn_motion_followed(on[k], tag.has && valid, kept, tag.gen, kept_gen, geo_gen);
    }

private:
    /* the kept vertices become (a copy of) the current ones, all of them, or none: the range is empty */
    bool keep_all(bool has_vertices)
    {
        kept_gen = geo_gen; lo = 0; hi = 0;
        kept = (on[0] || on[1]) && has_vertices;
        return kept;
    }
};
} // namespace rt
