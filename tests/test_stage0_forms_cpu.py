"""csrc/stage0_forms.h on the CPU: which form of k_generate_candidate and of k_temporal a call launches, or why it is refused.

The header is plain C++17 with no HIP include, so g++ compiles what hipcc compiles. The program below holds, beside the walk, a VERBATIM
restatement of the decision launch_generate and rt_temporal_resampling made before the header existed: the two macros GEN_LAUNCH and
GEN_LAUNCH_RP, the if chain over their call sites, the k_temporal chain and every refusal in its order, with each launch replaced by a
record of the template arguments (the kernel's defaults included) and of the tables the scene view passed to it was bound to. It is
compiled twice, plain and with -DRT_EXPERIMENTS, and walks EVERY combination of the inputs: 2^15 for stage 0, 2^4 for the temporal call.

One difference is wanted: a fused launch with the shadowed target function that is asked to trace the primary rays was launched in a form
that never writes the G-buffer, and is now refused. No caller asks for it (use_fused_stage0 requires the unshadowed target function
and is the only source of a non-null raycast_vis). The walk counts these inputs apart; every other input has to agree.

The second half holds the libraries to the tables: the instantiations of the two kernels in librestir_rt.so and librestir_rt_exp.so
are exactly the rows the program prints.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "stage0_forms.h"

/* ---- what the restated code needs of restir_rt.hip: the fields it read, the launches as records ---- */
enum { RT_LIGHTS_UNIFORM = 0, RT_LIGHTS_POWER = 1 }; /* include/restir_rt.h */
enum { T_UNIFORM = 0, T_POWER = 1, T_GRID = 2 };
struct SceneView { int lights = T_UNIFORM; bool with_grid = false; };
struct SceneViewGrid : SceneView { SceneViewGrid() { with_grid = true; } };
struct old_options { int ris_sample_count; bool use_shadowed_target_function; };
struct old_ctx
{
    int n_lights, grid_cells, light_mode;
    old_options opt;
    bool grid_built, alias_ok, temporal_unbiased, tune_defer_vis, tune_ris_pipe, says_motion, says_camera, ws;
    struct { bool ok; } h_grid;
    int d_lights_grid = T_GRID, d_lights_power = T_POWER;
    const char* err = nullptr;
};
struct Record
{
    int code = RT_OK;
    const char* err = "";
    int launches = 0;                    /* of k_generate_candidate / k_temporal: 1 wherever the call is not refused */
    bool t[10] = {};                     /* the template arguments */
    int tables = -1;                     /* what the scene view's light table was bound to */
    bool with_grid = false;              /* the launch took the SceneViewGrid */
    bool unbiased = false, queue = false; /* k_temporal_unbiased / k_candidate_visibility followed */
    bool tagged = false;                 /* the destination was tagged before the call returned */
};
static Record* REC;
#define RT_FAIL(ctx, code, msg) do { (ctx)->err = msg; return (code); } while (0)
static bool history_motion(const old_ctx* c) { return c->says_motion; }
static bool history_camera(const old_ctx* c) { return c->says_camera; }
static bool use_ws(const old_ctx* c, int) { return c->ws; }
static void tag_reservoir(old_ctx*) { REC->tagged = true; }
/* the kernel's template head as it is in frame_kernels.h, defaults included; the body records */
template <bool FUSE_TEMPORAL, bool SHADOWED, bool DEFER = false, bool PIPE = false, bool WS = false, bool RAYCAST = false, bool POWER = false, bool REPROJECT = false, bool MOTION = false, bool GRID = false>
static void k_generate_candidate(const SceneView& S)
{
    const bool t[10] = {FUSE_TEMPORAL, SHADOWED, DEFER, PIPE, WS, RAYCAST, POWER, REPROJECT, MOTION, GRID};
    memcpy(REC->t, t, sizeof(t));
    REC->tables = S.lights; REC->with_grid = S.with_grid; ++REC->launches;
}
template <bool SHADOWED, bool REPROJECT = false, bool MOTION = false>
static void k_temporal()
{
    REC->t[0] = SHADOWED; REC->t[1] = REPROJECT; REC->t[2] = MOTION; ++REC->launches;
}

/* ---- launch_generate as it was (restir_rt.hip before stage0_forms.h), restated verbatim ---- */
static int old_launch_generate(old_ctx* c, bool fuse, const void* raycast_vis)
{
    if (c->n_lights == 0 && c->opt.ris_sample_count > 0)
        RT_FAIL(c, RT_ERR_STATE, "scene has no emissive triangle (the reference divides by zero here)");
    SceneView S;
    const bool grid = c->grid_cells > 0 && c->opt.ris_sample_count > 0;
    SceneViewGrid SG;
    if (grid)
    {
        if (!c->grid_built || !c->h_grid.ok) RT_FAIL(c, RT_ERR_STATE, "rt_light_grid: no light of the scene has a positive finite area x luminance");
        S.lights = c->d_lights_grid;
    }
    SG.lights = S.lights; /* static_cast<SceneView&>(SG) = S */
    const bool power = !grid && c->light_mode == RT_LIGHTS_POWER && c->opt.ris_sample_count > 0;
    if (power)
    {
        if (!c->alias_ok) RT_FAIL(c, RT_ERR_STATE, "rt_light_sampling: no light of the scene has a positive finite area x luminance");
        S.lights = c->d_lights_power;
    }
    const bool sh = c->opt.use_shadowed_target_function;
    const bool mo = fuse && history_motion(c);
    const bool rp = mo || (fuse && history_camera(c));
    const bool ub = rp && !mo && c->temporal_unbiased;
    if (ub && sh) RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_unbiased: the shadowed target function is not built for the 1/Z merge");
    tag_reservoir(c);
    const int g = 0;
#define GEN_LAUNCH(FT, SH, DF, PP, WS_, RC, ...)                                                                                  \
    do {                                                                                                                          \
        if (grid && !(DF) && !(PP)) { const SceneViewGrid& S = SG; k_generate_candidate<FT, SH, false, false, WS_, RC, false, false, false, true>(__VA_ARGS__); break; } \
        if (power) k_generate_candidate<FT, SH, DF, PP, WS_, RC, true>(__VA_ARGS__);              \
        else k_generate_candidate<FT, SH, DF, PP, WS_, RC>(__VA_ARGS__);                          \
    } while (0)
#define GEN_LAUNCH_RP(SH, WS_, RC, ...)                                                                                           \
    do {                                                                                                                          \
        if (!rp) GEN_LAUNCH(true, SH, false, false, WS_, RC, __VA_ARGS__);                                                         \
        else if (mo && grid) { const SceneViewGrid& S = SG; k_generate_candidate<true, SH, false, false, WS_, RC, false, true, true, true>(__VA_ARGS__); } \
        else if (grid) { const SceneViewGrid& S = SG; k_generate_candidate<true, SH, false, false, WS_, RC, false, true, false, true>(__VA_ARGS__); } \
        else if (mo && power) k_generate_candidate<true, SH, false, false, WS_, RC, true, true, true>(__VA_ARGS__); \
        else if (mo) k_generate_candidate<true, SH, false, false, WS_, RC, false, true, true>(__VA_ARGS__); \
        else if (power) k_generate_candidate<true, SH, false, false, WS_, RC, true, true>(__VA_ARGS__); \
        else k_generate_candidate<true, SH, false, false, WS_, RC, false, true>(__VA_ARGS__);     \
    } while (0)
#ifdef RT_EXPERIMENTS
    if (grid && fuse && !sh && (c->tune_defer_vis || c->tune_ris_pipe))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_light_grid: the [exp] stage-0 variants (rt_tuning keys 11 and 12) are not built for the light grid");
    if (rp && fuse && ((!sh && c->tune_defer_vis) || (!sh && c->tune_ris_pipe)))
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_reprojection / rt_temporal_motion: the [exp] stage-0 variants (rt_tuning keys 11 and 12) gather their history from the own pixel only");
    if (fuse && !sh && c->tune_defer_vis)
    {
        if (c->tune_ris_pipe) GEN_LAUNCH(true, false, true, true, false, false, S);
        else GEN_LAUNCH(true, false, true, false, false, false, S);
        REC->queue = true; /* k_candidate_visibility */
        return RT_OK;
    }
#endif
    if (fuse && sh) GEN_LAUNCH_RP(true, false, false, S);
#ifdef RT_EXPERIMENTS
    else if (fuse && c->tune_ris_pipe) GEN_LAUNCH(true, false, false, true, false, false, S);
#endif
    else if (fuse && use_ws(c, g) && raycast_vis)
        GEN_LAUNCH_RP(false, true, true, S);
    else if (raycast_vis) RT_FAIL(c, RT_ERR_STATE, "the one-launch stage 0 needs the product's fused candidate kernel");
    else if (fuse && use_ws(c, g)) GEN_LAUNCH_RP(false, true, false, S);
    else if (fuse) GEN_LAUNCH_RP(false, false, false, S);
    else if (sh) GEN_LAUNCH(false, true, false, false, false, false, S);
    else GEN_LAUNCH(false, false, false, false, false, false, S);
#undef GEN_LAUNCH_RP
#undef GEN_LAUNCH
    if (ub)
    {
        REC->unbiased = true; /* k_temporal_unbiased */
    }
    return RT_OK;
}

/* ---- rt_temporal_resampling's decision as it was, restated verbatim ---- */
static int old_temporal_resampling(old_ctx* c)
{
    const bool mo = history_motion(c);
    const bool rp = !mo && history_camera(c);
    const bool ub = rp && c->temporal_unbiased;
    if (ub && c->opt.use_shadowed_target_function)
        RT_FAIL(c, RT_ERR_UNSUPPORTED, "rt_temporal_unbiased: the shadowed target function is not built for the 1/Z merge");
    tag_reservoir(c);
    if (ub)
    {
        REC->unbiased = true; /* k_temporal_unbiased */
    }
    else if (mo && c->opt.use_shadowed_target_function)
        k_temporal<true, true, true>();
    else if (mo)
        k_temporal<false, true, true>();
    else if (rp && c->opt.use_shadowed_target_function)
        k_temporal<true, true>();
    else if (rp)
        k_temporal<false, true>();
    else if (c->opt.use_shadowed_target_function)
        k_temporal<true>();
    else
        k_temporal<false>();
    return RT_OK;
}

/* ---- the walk ---- */
static rt::GenForm gen_of(const bool* t) { return rt::GenForm{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9]}; }
template <class Row, size_t N> static int row_of(const Row (&rows)[N], const Row& f)
{
    for (size_t i = 0; i < N; ++i)
        if (rows[i] == f) return (int)i;
    return -1;
}
enum { STAGE0_BITS = 15, TEMPORAL_BITS = 4 };
/* out: {inputs walked, differences that are not the wanted one, the wanted ones (refused now with the one-launch message), inputs with
 * fuse && shadowed && raycast_vis that the old code launched, forms selected by either side that are no row, rows no input selects,
 * rows, inputs the old code refused after it had tagged the destination} */
extern "C" void walk_stage0(int* out)
{
    int differ = 0, wanted = 0, expected = 0, no_row = 0, late = 0;
    std::vector<int> hits(rt::GEN_FORM_COUNT, 0);
    for (unsigned m = 0; m < (1u << STAGE0_BITS); ++m)
    {
        const auto bit = [m](int k) { return ((m >> k) & 1u) != 0; };
        old_ctx c = {};
        c.n_lights = bit(0) ? 0 : 7; c.opt.ris_sample_count = bit(1) ? 4 : 0;
        c.grid_cells = bit(2) ? 8 : 0; c.grid_built = bit(3); c.h_grid.ok = bit(4);
        c.light_mode = bit(5) ? RT_LIGHTS_POWER : RT_LIGHTS_UNIFORM; c.alias_ok = bit(6);
        c.opt.use_shadowed_target_function = bit(7);
        const bool fuse = bit(8);
        c.says_motion = bit(9); c.says_camera = bit(10); c.temporal_unbiased = bit(11);
        c.tune_defer_vis = bit(12); c.tune_ris_pipe = bit(13); c.ws = bit(14);
        for (int rc = 0; rc <= 1; ++rc)
        {
            Record o;
            REC = &o;
            o.code = old_launch_generate(&c, fuse, rc ? &c : nullptr);
            if (o.code != RT_OK) o.err = c.err;
            /* the inputs as launch_generate fills them: history_camera is not asked where history_motion said yes */
            rt::Stage0Inputs in = {};
            in.no_lights = c.n_lights == 0; in.ris = c.opt.ris_sample_count > 0;
            in.grid_on = c.grid_cells > 0; in.grid_ok = c.grid_built && c.h_grid.ok;
            in.power_on = c.light_mode == RT_LIGHTS_POWER; in.alias_ok = c.alias_ok;
            in.shadowed = c.opt.use_shadowed_target_function; in.fuse = fuse;
            in.history_motion = fuse && history_motion(&c);
            in.history_camera = fuse && !in.history_motion && history_camera(&c);
            in.temporal_unbiased = c.temporal_unbiased; in.defer_vis = c.tune_defer_vis; in.ris_pipe = c.tune_ris_pipe;
            in.ws = use_ws(&c, 0); in.raycast = rc != 0;
            const rt::Stage0Plan p = rt::stage0_plan(in);
            bool same = p.code == o.code && strcmp(rt::FORM_MESSAGE[p.why], o.err) == 0 && (p.why == rt::FORM_OK) == (p.code == RT_OK);
            if (same && p.code == RT_OK)
                same = o.launches == 1 && p.form == gen_of(o.t) && (int)p.tables == o.tables && p.form.grid == o.with_grid &&
                       p.unbiased_merge == o.unbiased && p.deferred_queue == o.queue;
            const bool case_3b = fuse && in.shadowed && in.raycast && o.code == RT_OK;
            if (case_3b) ++expected;
            if (!same)
            {
                if (case_3b && p.code == RT_ERR_STATE && p.why == rt::REFUSE_ONE_LAUNCH) ++wanted;
                else ++differ;
            }
            if (o.code == RT_OK && row_of(rt::GEN_FORMS, gen_of(o.t)) < 0) ++no_row;
            if (p.code == RT_OK)
            {
                const int r = row_of(rt::GEN_FORMS, p.form);
                if (r < 0) ++no_row; else ++hits[r];
            }
            if (o.code != RT_OK && o.tagged) ++late;
        }
    }
    int dead = 0;
    for (int h : hits) dead += h == 0;
    out[0] = 2 << STAGE0_BITS; out[1] = differ; out[2] = wanted; out[3] = expected; out[4] = no_row; out[5] = dead;
    out[6] = (int)rt::GEN_FORM_COUNT; out[7] = late;
}
/* out: {inputs walked, differences, forms that are no row, rows no input selects, rows} */
extern "C" void walk_temporal(int* out)
{
    int differ = 0, no_row = 0;
    constexpr size_t ROWS = sizeof(rt::TEMPORAL_FORMS) / sizeof(rt::TemporalForm);
    std::vector<int> hits(ROWS, 0);
    for (unsigned m = 0; m < (1u << TEMPORAL_BITS); ++m)
    {
        old_ctx c = {};
        c.opt.use_shadowed_target_function = m & 1; c.says_motion = m & 2; c.says_camera = m & 4; c.temporal_unbiased = m & 8;
        Record o;
        REC = &o;
        o.code = old_temporal_resampling(&c);
        if (o.code != RT_OK) o.err = c.err;
        rt::TemporalInputs in = {};
        in.shadowed = c.opt.use_shadowed_target_function; in.temporal_unbiased = c.temporal_unbiased;
        in.history_motion = history_motion(&c);
        in.history_camera = !in.history_motion && history_camera(&c);
        const rt::TemporalPlan p = rt::temporal_plan(in);
        bool same = p.code == o.code && strcmp(rt::FORM_MESSAGE[p.why], o.err) == 0 && (p.why == rt::FORM_OK) == (p.code == RT_OK) && (p.code == RT_OK) == o.tagged;
        if (same && p.code == RT_OK) same = p.unbiased_merge == o.unbiased && o.launches == (o.unbiased ? 0 : 1);
        if (same && p.code == RT_OK && !p.unbiased_merge)
        {
            const rt::TemporalForm f = {o.t[0], o.t[1], o.t[2]};
            same = p.form == f;
            const int r = row_of(rt::TEMPORAL_FORMS, p.form);
            if (r < 0 || row_of(rt::TEMPORAL_FORMS, f) < 0) ++no_row; else ++hits[r];
        }
        if (!same) ++differ;
    }
    int dead = 0;
    for (int h : hits) dead += h == 0;
    out[0] = 1 << TEMPORAL_BITS; out[1] = differ; out[2] = no_row; out[3] = dead; out[4] = (int)ROWS;
}
/* the tables as the demangled names of the instantiations, one per line */
extern "C" const char* tables()
{
    static std::string s;
    s.clear();
    const auto b = [](bool v) { return v ? "true" : "false"; };
    for (const rt::GenForm& f : rt::GEN_FORMS)
        s += std::string("k_generate_candidate<") + b(f.fuse) + ", " + b(f.shadowed) + ", " + b(f.defer) + ", " + b(f.pipe) + ", " + b(f.ws) + ", " +
             b(f.raycast) + ", " + b(f.power) + ", " + b(f.reproject) + ", " + b(f.motion) + ", " + b(f.grid) + ">\n";
    for (const rt::TemporalForm& f : rt::TEMPORAL_FORMS)
        s += std::string("k_temporal<") + b(f.shadowed) + ", " + b(f.reproject) + ", " + b(f.motion) + ">\n";
    return s.c_str();
}
"""

_results = {}


def walk(exp):
    """the program compiled plain (the product's library) or with -DRT_EXPERIMENTS, walked once"""
    if exp not in _results:
        d = tempfile.mkdtemp(prefix="stage0_forms_")
        src, so = os.path.join(d, "stage0_forms.cpp"), os.path.join(d, "stage0_forms.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src]
                       + (["-DRT_EXPERIMENTS"] if exp else []), check=True, capture_output=True, timeout=300)
        lib = C.CDLL(so)
        s0, t = (C.c_int * 8)(), (C.c_int * 5)()
        lib.walk_stage0(s0)
        lib.walk_temporal(t)
        lib.tables.restype = C.c_char_p
        r = dict(zip(("inputs", "differ", "wanted", "expected", "no_row", "dead", "rows", "late"), s0))
        r["temporal"] = dict(zip(("inputs", "differ", "no_row", "dead", "rows"), t))
        r["tables"] = set(lib.tables().decode().split("\n")) - {""}
        _results[exp] = r
    return _results[exp]


BUILDS = pytest.mark.parametrize("exp", [False, True], ids=["product", "exp"])


@BUILDS
def test_plan_equals_the_restated_chain_for_every_input(exp):
    """launch or refuse, the code, the message, the form, the bound tables and the two follow-up flags agree for every input but the
    wanted difference, and the walk visits all 2^15 x 2 inputs"""
    w = walk(exp)
    assert w["inputs"] == 65536
    assert w["differ"] == 0


@BUILDS
def test_the_only_difference_is_the_fused_shadowed_launch_with_primary_rays(exp):
    """every input with fuse && shadowed && raycast_vis that the old code launched (in a form that writes no G-buffer) is refused
    with the one-launch message, and no other input differs: a condition on the count, not a tolerance"""
    w = walk(exp)
    assert w["expected"] > 0
    assert w["wanted"] == w["expected"]


@BUILDS
def test_every_selected_form_is_a_row_and_every_row_is_selected(exp):
    """42 forms in the product, 48 with the [exp] ones; no form either side selects is missing from the table, no row is dead"""
    w = walk(exp)
    assert w["rows"] == (48 if exp else 42)
    assert (w["no_row"], w["dead"]) == (0, 0)
    assert w["temporal"]["rows"] == 6
    assert (w["temporal"]["no_row"], w["temporal"]["dead"]) == (0, 0)


@BUILDS
def test_temporal_plan_equals_the_restated_chain_for_every_input(exp):
    """rt_temporal_resampling: its six k_temporal arms, its k_temporal_unbiased arm and its refusal, over all 2^4 inputs; it tagged
    the buffer exactly where it did not refuse, as it does now"""
    t = walk(exp)["temporal"]
    assert t["inputs"] == 16
    assert t["differ"] == 0


def test_refusals_came_after_the_tag_only_in_the_experiments_build_and_for_the_one_launch_message():
    """what moving every refusal before the side effects changes: the product's library refused after the tag with the one-launch
    message alone, the [exp] one with its three messages too; both counts are of inputs the walk has shown to be refused alike"""
    assert 0 < walk(False)["late"] < walk(True)["late"]


def instantiations(path):
    """the demangled k_generate_candidate / k_temporal instantiations named in a library (as tests/test_abi.py reads kernel names)"""
    out = subprocess.run(["strings", "-a", path], capture_output=True, text=True, check=True).stdout
    names = sorted(set(re.findall(r"^_Z\d+(?:k_generate_candidate|k_temporal)I\w+$", out, re.M)))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {re.match(r"void (k_\w+<[^<>]*>)\(", d).group(1) for d in dem}


@BUILDS
def test_library_carries_exactly_the_tables_forms(exp):
    """a row launches its own instantiation and nothing else instantiates the two kernels: the set of instantiations in the
    library is the set of rows"""
    from cedec_2024_rt_amd import api

    path = api.EXP_LIB_PATH if exp else api.LIB_PATH
    if not os.path.exists(path):
        pytest.skip(os.path.basename(path) + " is not built")
    assert instantiations(path) == walk(exp)["tables"]
