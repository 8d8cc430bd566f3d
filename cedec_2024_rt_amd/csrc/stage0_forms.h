/* stage0_forms.h — which form of k_generate_candidate and of k_temporal a call launches, or why it is refused.
 * The tables below are the ONLY place that names a form: restir_rt.hip instantiates and launches a kernel from the row that equals the
 * plan's form, and nothing else. Host only, plain C++17, no HIP include: tests/test_stage0_forms_cpu.py walks every input beside the
 * macros and if chains this header replaced, and holds the libraries' instantiations to the tables. */
#pragma once
#include <cstddef>

#include "../../include/restir_rt.h"

namespace rt
{
/* k_generate_candidate's template parameters, in their order (frame_kernels.h explains each above the kernel) */
struct GenForm
{
    bool fuse, shadowed, defer, pipe, ws, raycast, power, reproject, motion, grid;
    constexpr bool operator==(const GenForm& o) const
    {
        return fuse == o.fuse && shadowed == o.shadowed && defer == o.defer && pipe == o.pipe && ws == o.ws && raycast == o.raycast &&
               power == o.power && reproject == o.reproject && motion == o.motion && grid == o.grid;
    }
};
/* the kernel's five static_asserts */
constexpr bool gen_form_valid(GenForm f)
{
    return (!f.defer || (f.fuse && !f.shadowed)) && (!f.raycast || (f.ws && f.fuse && !f.shadowed && !f.defer && !f.pipe)) &&
           (!f.reproject || (f.fuse && !f.defer && !f.pipe)) && (!f.motion || f.reproject) && (!f.grid || (!f.power && !f.defer && !f.pipe));
}
enum LightTables { LIGHTS_UNIFORM, LIGHTS_POWER, LIGHTS_GRID };  /* rt_light_sampling, rt_light_grid: whose light table and radiance */
enum History { HISTORY_OWN_PIXEL, HISTORY_REPROJECT, HISTORY_MOTION }; /* rt_temporal_reprojection, rt_temporal_motion */
constexpr GenForm gen_form(GenForm base, int lights, int history)
{
    base.power = lights == LIGHTS_POWER; base.grid = lights == LIGHTS_GRID;
    base.reproject = history != HISTORY_OWN_PIXEL; base.motion = history == HISTORY_MOTION;
    return base;
}
/* <fuse, shadowed, defer, pipe, ws, raycast>: a new form of the kernel is a row here */
constexpr GenForm GEN_BASES[] = {
#ifdef RT_EXPERIMENTS
    {true, false, true, true, false, false},  /* [exp] rt_tuning 11 and 12 */
    {true, false, true, false, false, false}, /* [exp] rt_tuning 11: the visibility-reuse rays through a queue */
#endif
    {true, true, false, false, false, false}, /* candidates + temporal with the shadowed target function */
#ifdef RT_EXPERIMENTS
    {true, false, false, true, false, false}, /* [exp] rt_tuning 12: the pipelined RIS loop */
#endif
    {true, false, false, false, true, true},    /* the whole frame's stage 0 in one launch: primary ray + candidates + temporal */
    {true, false, false, false, true, false},   /* candidates + temporal (strips, rt_timing) */
    {true, false, false, false, false, false},  /* ... without the work-sharing walk (rt_tuning 13 = 0) */
    {false, true, false, false, false, false},  /* rt_generate_candidate with the shadowed target function */
    {false, false, false, false, false, false}, /* rt_generate_candidate */
};
/* {lights, history}: the bases above and these are in the order in which the code object has held the kernels since each was added,
 * so that a resource table or a profile of this build lists them where the recorded ones do */
constexpr int GEN_VARIANTS[9][2] = {{LIGHTS_GRID, HISTORY_OWN_PIXEL},  {LIGHTS_POWER, HISTORY_OWN_PIXEL}, {LIGHTS_UNIFORM, HISTORY_OWN_PIXEL},
                                    {LIGHTS_GRID, HISTORY_MOTION},     {LIGHTS_GRID, HISTORY_REPROJECT},  {LIGHTS_POWER, HISTORY_MOTION},
                                    {LIGHTS_UNIFORM, HISTORY_MOTION},  {LIGHTS_POWER, HISTORY_REPROJECT}, {LIGHTS_UNIFORM, HISTORY_REPROJECT}};
/* every base in every light selection and with every history that the kernel's static_asserts allow: all nine for the product's fused
 * forms, the three light selections for the unfused ones, uniform and power for the [exp] ones */
template <size_t N> struct GenFormRows
{
    GenForm row[N] = {};
    size_t n = 0;
    constexpr void add(GenForm f) /* once */
    {
        for (size_t i = 0; i < n; ++i)
            if (row[i] == f) return;
        row[n++] = f;
    }
};
template <size_t N> constexpr GenFormRows<N> gen_form_rows()
{
    GenFormRows<N> t;
#ifdef RT_EXPERIMENTS
    /* where the experiments library's code object has held this form since r33: in front of the [exp] ones */
    t.add(gen_form({true, false, false, false, false, false}, LIGHTS_GRID, HISTORY_OWN_PIXEL));
#endif
    for (const GenForm& b : GEN_BASES)
        for (const auto& v : GEN_VARIANTS)
            if (gen_form_valid(gen_form(b, v[0], v[1]))) t.add(gen_form(b, v[0], v[1]));
    return t;
}
constexpr size_t GEN_FORM_COUNT = gen_form_rows<9 * sizeof(GEN_BASES) / sizeof(GenForm)>().n;
constexpr GenFormRows<GEN_FORM_COUNT> GEN_FORM_ROWS = gen_form_rows<GEN_FORM_COUNT>();
static constexpr const GenForm (&GEN_FORMS)[GEN_FORM_COUNT] = GEN_FORM_ROWS.row; /* static: a reference would be of external linkage */

/* k_temporal's template parameters (rt_temporal_resampling) */
struct TemporalForm
{
    bool shadowed, reproject, motion;
    constexpr bool operator==(const TemporalForm& o) const { return shadowed == o.shadowed && reproject == o.reproject && motion == o.motion; }
};
constexpr TemporalForm TEMPORAL_FORMS[] = {{true, true, true},  {false, true, true},  {true, true, false},
                                           {false, true, false}, {true, false, false}, {false, false, false}};

template <class Row, size_t N, class Valid> constexpr bool forms_valid(const Row (&rows)[N], Valid valid)
{
    for (const Row& r : rows)
        if (!valid(r)) return false;
    return true;
}
template <class Row, size_t N> constexpr bool forms_differ(const Row (&rows)[N])
{
    for (size_t i = 0; i < N; ++i)
        for (size_t k = i + 1; k < N; ++k)
            if (rows[i] == rows[k]) return false;
    return true;
}
static_assert(forms_valid(GEN_FORMS, gen_form_valid), "GEN_FORMS: a row that k_generate_candidate's static_asserts refuse");
static_assert(forms_differ(GEN_FORMS), "GEN_FORMS: a form occurs twice");
static_assert(forms_differ(TEMPORAL_FORMS), "TEMPORAL_FORMS: a form occurs twice");

/* why a call is refused; FORM_MESSAGE[why] is the text rt_last_error gives */
enum FormRefusal
{
    FORM_OK,
    REFUSE_NO_LIGHT,
    REFUSE_GRID_NO_LIGHT,
    REFUSE_POWER_NO_LIGHT,
    REFUSE_UNBIASED_SHADOWED,
    REFUSE_EXP_GRID,
    REFUSE_EXP_REPROJECT,
    REFUSE_ONE_LAUNCH,
};
constexpr const char* FORM_MESSAGE[] = {
    "",
    "scene has no emissive triangle (the reference divides by zero here)",
    "rt_light_grid: no light of the scene has a positive finite area x luminance",
    "rt_light_sampling: no light of the scene has a positive finite area x luminance",
    "rt_temporal_unbiased: the shadowed target function is not built for the 1/Z merge",
    "rt_light_grid: the [exp] stage-0 variants (rt_tuning keys 11 and 12) are not built for the light grid",
    "rt_temporal_reprojection / rt_temporal_motion: the [exp] stage-0 variants (rt_tuning keys 11 and 12) gather their history from the own pixel only",
    "the one-launch stage 0 needs the product's fused candidate kernel",
};

/* everything launch_generate decides on */
struct Stage0Inputs
{
    bool no_lights, ris;           /* n_lights == 0, ris_sample_count > 0 */
    bool grid_on, grid_ok;         /* rt_light_grid on; its tables are built and usable */
    bool power_on, alias_ok;       /* rt_light_sampling = RT_LIGHTS_POWER; its alias table is usable */
    bool shadowed, fuse;           /* use_shadowed_target_function; the launch merges the history */
    bool history_motion, history_camera; /* what the two functions of restir_rt.hip said of the history buffer */
    bool temporal_unbiased, defer_vis, ris_pipe, ws, raycast; /* rt_temporal_unbiased, rt_tuning 11 / 12 / 13, the launch traces the primary rays */
};
/* code != RT_OK: refused, for the reason `why`. Otherwise the form, whose tables it reads, and what follows the launch:
 * unbiased_merge: it runs under a history camera of NaNs and k_temporal_unbiased merges the history after it;
 * deferred_queue: [exp] it fills the queue that k_candidate_visibility walks after it */
struct Stage0Plan
{
    int code;
    FormRefusal why;
    GenForm form;
    LightTables tables;
    bool unbiased_merge, deferred_queue;
};
constexpr Stage0Plan stage0_refusal(int code, FormRefusal why) { return {code, why, {}, LIGHTS_UNIFORM, false, false}; }
constexpr Stage0Plan stage0_plan(const Stage0Inputs& in)
{
    if (in.no_lights && in.ris) return stage0_refusal(RT_ERR_STATE, REFUSE_NO_LIGHT);
    /* rt_light_grid decides the selection while it is on; rt_light_sampling's mode is kept and applies again when it goes off */
    const bool grid = in.grid_on && in.ris, power = !grid && in.power_on && in.ris;
    if (grid && !in.grid_ok) return stage0_refusal(RT_ERR_STATE, REFUSE_GRID_NO_LIGHT);
    if (power && !in.alias_ok) return stage0_refusal(RT_ERR_STATE, REFUSE_POWER_NO_LIGHT);
    /* a motion launch is a reprojecting one. rt_temporal_unbiased: a reprojecting launch becomes two, the candidates without the merge
     * and k_temporal_unbiased in place on their buffer; a motion launch cannot be one, the two toggles refuse each other */
    const bool mo = in.fuse && in.history_motion, rp = mo || (in.fuse && in.history_camera), ub = rp && !mo && in.temporal_unbiased;
    if (ub && in.shadowed) return stage0_refusal(RT_ERR_UNSUPPORTED, REFUSE_UNBIASED_SHADOWED);
    bool defer = false, pipe = false;
#ifdef RT_EXPERIMENTS
    const bool exp = in.fuse && !in.shadowed && (in.defer_vis || in.ris_pipe);
    if (exp && grid) return stage0_refusal(RT_ERR_UNSUPPORTED, REFUSE_EXP_GRID);
    if (exp && rp) return stage0_refusal(RT_ERR_UNSUPPORTED, REFUSE_EXP_REPROJECT);
    defer = exp && in.defer_vis; pipe = exp && in.ris_pipe;
#endif
    /* the work-sharing walk, and the primary rays with it, in the product's fused unshadowed kernel only; the [exp] forms have
     * always ignored raycast */
    const bool ws = in.fuse && !in.shadowed && !defer && !pipe && in.ws;
    if (in.raycast && !ws && !defer && !pipe) return stage0_refusal(RT_ERR_STATE, REFUSE_ONE_LAUNCH);
    return {RT_OK, FORM_OK, {in.fuse, in.shadowed, defer, pipe, ws, ws && in.raycast, power, rp, mo, grid},
            grid ? LIGHTS_GRID : (power ? LIGHTS_POWER : LIGHTS_UNIFORM), ub, defer};
}

/* rt_temporal_resampling: k_temporal's form, or k_temporal_unbiased wherever the history is gathered by reprojection (not by motion) */
struct TemporalInputs { bool shadowed, history_motion, history_camera, temporal_unbiased; };
struct TemporalPlan
{
    int code;
    FormRefusal why;
    TemporalForm form;
    bool unbiased_merge;
};
constexpr TemporalPlan temporal_plan(const TemporalInputs& in)
{
    const bool mo = in.history_motion, rp = !mo && in.history_camera, ub = rp && in.temporal_unbiased;
    if (ub && in.shadowed) return {RT_ERR_UNSUPPORTED, REFUSE_UNBIASED_SHADOWED, {}, false};
    if (ub) return {RT_OK, FORM_OK, {}, true};
    return {RT_OK, FORM_OK, {in.shadowed, mo || rp, mo}, false};
}
} // namespace rt
