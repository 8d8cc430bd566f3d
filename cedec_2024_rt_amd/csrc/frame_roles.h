/* frame_roles.h — which physical reservoir buffer plays which part in a staged frame (restir_rt.hip: rt_frame_stage_begin / _run / _end and
 * the take of the look-ahead stage 0). Host only, plain C++17, no HIP include: tests/test_frame_roles_cpu.py walks every reachable state. */
#pragma once
namespace rt
{
enum { ROLE_RES_0 = 0, ROLE_RES_1 = 1, ROLE_RES_TEMPORAL = 2 }; /* RT_RES_* of include/restir_rt.h (restir_rt.hip asserts it) */
struct FrameRoles
{
    /* three reservoir buffers carry the reference's names (res_map); a fourth, allocated when the pipelined stage 0 is
     * first used, receives the NEXT frame's candidates while this frame's passes still read the other three */
    /* r05: and a fifth. The buffer the previous frame's resolve reads ("quarantine") is not handed to the look-ahead candidates
     * until one more frame has passed: they get the buffer that left the roles a frame earlier (last reader: two tails back). */
    int res_map[3] = {0, 1, 2};
    int spare = 3;      /* physical buffer not named by res_map: the look-ahead candidates' */
    int quarantine = 4; /* the buffer that left the roles at the last take (the previous frame's final one, or a free one) */
    /* X = history, Y = candidates(+temporal) -> next history, Z = spatial ping-pong partner; in / out: what the running stage reads / writes;
     * final_res: the logical name of the buffer the last frame resolved */
    int X = 0, Y = 1, Z = 2, in = 0, out = 1, final_res = ROLE_RES_1;
};
/* stage 0 begins: the roles from the logical names */
inline void roles_begin(FrameRoles& r) { r.X = r.res_map[ROLE_RES_TEMPORAL]; r.Y = r.res_map[ROLE_RES_0]; r.Z = r.res_map[ROLE_RES_1]; r.in = r.Y; r.out = r.Z; }
/* this frame's candidates are in the spare buffer already: it becomes Y (stage 0's generate is skipped;
 * rt_frame_stage_output / _end see the swapped roles). Of the two buffers the passes ping-pong through, the one the
 * previous frame's resolve may still be reading on the tail stream (its final buffer) becomes the new spare — the
 * pipelined stage 0 after next waits for the tail anyway — and pass 0 writes the other one, so that no spatial pass
 * of this frame has to wait for the previous frame's resolve. With no spatial pass, logical RES_1 keeps its buffer
 * (the reference resolves a buffer that frame did not write: its content must carry over). */
inline void roles_take(FrameRoles& r, int passes, bool spec_free)
{
    const int r0 = r.Y, r1 = r.Z;
    const int prev_final = r.res_map[r.final_res == ROLE_RES_1 ? ROLE_RES_1 : ROLE_RES_0];
    r.Y = r.spare;
    int freed = r0;
    if (passes >= 1 && prev_final == r1) { r.Z = r0; freed = r1; }
    /* r05: the freed buffer (the previous frame's final one, or one nobody reads) waits a frame in quarantine; the look-ahead
     * candidates of the NEXT frame go to the buffer freed a frame earlier. RT_TUNING 22 = 0: the freed one at once (r04). */
    if (spec_free) { r.spare = r.quarantine; r.quarantine = freed; }
    else r.spare = freed;
    r.in = r.Y; r.out = r.Z;
}
/* buffer roles are a pure function of the stage index, so a repeated _begin (retry after a failed
 * _run) cannot swap the ping-pong pair twice: pass k reads what pass k-1 wrote (Y for k = 0) and
 * writes Z for even k, X for odd k */
inline void roles_pass(FrameRoles& r, int k) { r.in = (k == 0) ? r.Y : ((k & 1) ? r.Z : r.X); r.out = (k & 1) ? r.X : r.Z; }
/* the buffer the frame resolves: the last pass's output, or Z with no pass at all */
inline int roles_final_phys(const FrameRoles& r, int passes) { return passes > 0 ? r.out : r.Z; }
/* the frame ends. New logical names: TEMPORAL = Y; RES_1 = Z; RES_0 = X (pass-1 output / copy) */
inline void roles_end(FrameRoles& r, int passes)
{
    const int X = r.X, Y = r.Y, Z = r.Z, final_phys = roles_final_phys(r, passes);
    r.res_map[ROLE_RES_TEMPORAL] = Y; r.res_map[ROLE_RES_0] = X; r.res_map[ROLE_RES_1] = Z;
    r.final_res = (final_phys == Z) ? ROLE_RES_1 : ROLE_RES_0;
}
/* the look-ahead candidates' buffer has no role in the running frame, is not in quarantine and is not `guarded` (the buffer a tail in
 * flight reads where nothing else orders the look-ahead behind it; -1: none) */
inline bool roles_spare_free(const FrameRoles& r, int guarded) { return r.spare != r.X && r.spare != r.Y && r.spare != r.Z && r.spare != r.quarantine && r.spare != guarded; }
} // namespace rt
