"""csrc/frame_roles.h on the CPU: which physical reservoir buffer is history, candidates, ping-pong partner, spare and quarantine.

The header is plain C++17 with no HIP include, so g++ compiles what hipcc compiles. The program below holds, beside the walk, a
VERBATIM restatement of the integer statements rt_frame_stage_begin, raycast_or_take, rt_frame_stage_end and launch_next_raycast
had before the header existed (the fields of rt_ctx they touched, under their old names). The walk visits EVERY state reachable
from the start state under every per-frame choice (spatial passes 0..8: the ping-pong of pass indices 3..7 is what a frame with more
passes than the reference's default runs, look-ahead free of the main stream or not, candidates taken
from the look-ahead or not) and compares the two after every begin, take, pass and end.
"""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <set>
#include <vector>
#include <array>
#include "frame_roles.h"

/* ---- the staged frame's role arithmetic as it was (restir_rt.hip before frame_roles.h), restated verbatim ---- */
enum { RT_RES_0 = 0, RT_RES_1 = 1, RT_RES_TEMPORAL = 2 }; /* include/restir_rt.h */
struct old_options { int spatial_resampling_passes; };
struct old_ctx
{
    int res_map[3] = {0, 1, 2};
    int spare = 3;
    int quarantine = 4;
    int fX = 0, fY = 1, fZ = 2, f_in = 0, f_out = 1, f_final = RT_RES_1;
    old_options opt = {0};
    bool tune_spec_free = false;
};
static bool spec_free(const old_ctx* c) { return c->tune_spec_free; }
static void old_begin(old_ctx* c)
{
    c->fX = c->res_map[RT_RES_TEMPORAL]; c->fY = c->res_map[RT_RES_0]; c->fZ = c->res_map[RT_RES_1];
    c->f_in = c->fY; c->f_out = c->fZ;
}
static void old_pass(old_ctx* c, int stage)
{
    const int passes = c->opt.spatial_resampling_passes;
    if (stage >= 1 && stage <= passes)
    {
        const int k = stage - 1;
        c->f_in = (k == 0) ? c->fY : ((k & 1) ? c->fZ : c->fX);
        c->f_out = (k & 1) ? c->fX : c->fZ;
    }
}
static void old_take(old_ctx* c)
{
            const int r0 = c->fY, r1 = c->fZ;
            const int prev_final = c->res_map[c->f_final == RT_RES_1 ? RT_RES_1 : RT_RES_0];
            c->fY = c->spare;
            int freed = r0;
            if (c->opt.spatial_resampling_passes >= 1 && prev_final == r1) { c->fZ = r0; freed = r1; }
            if (spec_free(c)) { c->spare = c->quarantine; c->quarantine = freed; }
            else c->spare = freed;
            c->f_in = c->fY; c->f_out = c->fZ;
}
static void old_end(old_ctx* c)
{
    const int passes = c->opt.spatial_resampling_passes;
    const int X = c->fX, Y = c->fY, Z = c->fZ;
    const int final_phys = passes > 0 ? c->f_out : Z;
    c->res_map[RT_RES_TEMPORAL] = Y;
    c->res_map[RT_RES_0] = X;
    c->res_map[RT_RES_1] = Z;
    c->f_final = (final_phys == Z) ? RT_RES_1 : RT_RES_0;
}
static bool old_spare_in_use(const old_ctx* c)
{
    return (c->spare == c->fX || c->spare == c->fY || c->spare == c->fZ || c->spare == c->quarantine);
}

/* ---- the walk ---- */
static bool same(const rt::FrameRoles& r, const old_ctx& o)
{
    return r.res_map[0] == o.res_map[0] && r.res_map[1] == o.res_map[1] && r.res_map[2] == o.res_map[2] && r.spare == o.spare &&
           r.quarantine == o.quarantine && r.X == o.fX && r.Y == o.fY && r.Z == o.fZ && r.in == o.f_in && r.out == o.f_out &&
           r.final_res == o.f_final;
}
static bool five_different(const rt::FrameRoles& r)
{
    const int b[5] = {r.X, r.Y, r.Z, r.spare, r.quarantine};
    int seen = 0;
    for (int v : b)
    {
        if (v < 0 || v > 4) return false;
        seen |= 1 << v;
    }
    return seen == 31;
}
typedef std::array<int, 6> Key; /* what one frame leaves to the next: res_map, spare, quarantine, final_res */
static Key key_of(const rt::FrameRoles& r) { return Key{r.res_map[0], r.res_map[1], r.res_map[2], r.spare, r.quarantine, r.final_res}; }

/* out: {states, transitions, differences from the restatement, takes after which the five roles were not five buffers,
 * stage-0 ends at which the candidates' buffer was not free, orders of the five buffers seen, values of final_res seen} */
extern "C" void walk(int* out)
{
    static_assert((int)rt::ROLE_RES_0 == RT_RES_0 && (int)rt::ROLE_RES_1 == RT_RES_1 && (int)rt::ROLE_RES_TEMPORAL == RT_RES_TEMPORAL, "names");
    int transitions = 0, differ = 0, not_five = 0, not_free = 0;
    const rt::FrameRoles start;
    if (!same(start, old_ctx())) ++differ; /* the start state: res_map {0, 1, 2}, spare 3, quarantine 4, final RT_RES_1 */
    std::set<Key> seen{key_of(start)};
    std::vector<rt::FrameRoles> todo{start};
    while (!todo.empty())
    {
        const rt::FrameRoles from = todo.back();
        todo.pop_back();
        for (int passes = 0; passes <= 8; ++passes)
            for (int free_ = 0; free_ <= 1; ++free_)
                for (int taken = 0; taken <= 1; ++taken)
                {
                    rt::FrameRoles r = from;
                    old_ctx o;
                    for (int k = 0; k < 3; ++k) o.res_map[k] = from.res_map[k];
                    o.spare = from.spare; o.quarantine = from.quarantine; o.f_final = from.final_res;
                    o.fX = from.X; o.fY = from.Y; o.fZ = from.Z; o.f_in = from.in; o.f_out = from.out;
                    o.opt.spatial_resampling_passes = passes; o.tune_spec_free = free_ != 0;
                    rt::roles_begin(r); old_begin(&o);
                    if (!same(r, o)) ++differ;
                    if (taken)
                    {
                        rt::roles_take(r, passes, free_ != 0); old_take(&o);
                        if (!same(r, o)) ++differ;
                        if (!five_different(r)) ++not_five;
                    }
                    /* the end of stage 0 launches the look-ahead: what launch_next_raycast checks there */
                    if (rt::roles_spare_free(r, -1) != !old_spare_in_use(&o)) ++differ;
                    if (!rt::roles_spare_free(r, -1)) ++not_free;
                    if (rt::roles_spare_free(r, r.spare)) ++differ; /* a guarded buffer is never free */
                    for (int stage = 1; stage <= passes + 1; ++stage) /* passes + 1: the resolve stage, no roles change */
                    {
                        if (stage <= passes) rt::roles_pass(r, stage - 1);
                        old_pass(&o, stage);
                        if (!same(r, o)) ++differ;
                    }
                    if (rt::roles_final_phys(r, passes) != (passes > 0 ? o.f_out : o.fZ)) ++differ;
                    rt::roles_end(r, passes); old_end(&o);
                    if (!same(r, o)) ++differ;
                    ++transitions;
                    if (seen.insert(key_of(r)).second) todo.push_back(r);
                }
    }
    std::set<std::array<int, 5>> orders;
    std::set<int> finals;
    for (const Key& k : seen) { orders.insert({k[0], k[1], k[2], k[3], k[4]}); finals.insert(k[5]); }
    out[0] = (int)seen.size(); out[1] = transitions; out[2] = differ; out[3] = not_five; out[4] = not_free;
    out[5] = (int)orders.size(); out[6] = (int)finals.size();
}
"""

_result = None


def walk():
    global _result
    if _result is None:
        d = tempfile.mkdtemp(prefix="frame_roles_")
        src, so = os.path.join(d, "frame_roles.cpp"), os.path.join(d, "frame_roles.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        lib = C.CDLL(so)
        out = (C.c_int * 7)()
        lib.walk(out)
        _result = dict(zip(("states", "transitions", "differ", "not_five", "not_free", "orders", "finals"), out))
    return _result


def test_header_equals_the_restated_statements_everywhere():
    """after every begin, take, pass and end of every transition the header's roles equal the restatement's in every field, and
    so do the final buffer and the "candidates' buffer is free" predicate"""
    assert walk()["differ"] == 0


def test_roles_are_five_different_buffers_after_every_take():
    """X, Y, Z, spare and quarantine name five different buffers after every take, and the look-ahead candidates' buffer is free
    at the end of every stage 0, taken or not: what launch_next_raycast otherwise finds out on a GPU"""
    w = walk()
    assert w["not_five"] == 0
    assert w["not_free"] == 0


def test_the_walk_closed_over_every_reachable_state():
    """5! orders of the buffers x 2 values of final_res = 240 states, 9 x 2 x 2 choices per state = 8 640 transitions: a walk that
    silently visits less does not pass"""
    w = walk()
    assert (w["orders"], w["finals"]) == (120, 2)
    assert w["states"] == 240
    assert w["transitions"] == 8640
