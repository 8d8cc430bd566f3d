"""The per-pixel record of remembered occluders (csrc/occluder_hint.h) on the CPU.

The header is RT_HD, so `g++` compiles the functions hipcc compiles (as tests/test_targeted_rays_cpu.py does for bvh_cull.h). The
program below drives them the way k_generate_candidate does: positions in order, only entries that name a triangle of the scene are
tested, the first that occludes the ray settles it (hint_hit); if none does and the walk names an occluder, hint_insert. One event =
(the set of triangles that occlude the ray, the triangle the walk would name). The records are compared with a Python model of
"most recently used first, no duplicates, N entries" after every event.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include "occluder_hint.h"
using namespace rt;

/* one ray against a record, as the candidates' kernel drives the header. occ: n_occ triangles that occlude the ray; walk: the
 * triangle the walk names if it runs (-1: the ray is visible). rec: N entries, updated in place. tested: the triangles tested, in order.
 * returns: tests | settled position + 1 << 8 | record changed << 16 | walk ran << 17 */
template <int N>
static int event(int* rec, int n_tris, const int* occ, int n_occ, int walk, int* tested)
{
    OccluderHints<N> h;
    for (int k = 0; k < N; ++k) h.tri[k] = rec[k];
    int n_tests = 0, at = -1;
    for (int k = 0; k < N; ++k)
    {
        if (at >= 0 || !hint_pending(h, k, n_tris)) continue;
        tested[n_tests++] = h.tri[k];
        for (int j = 0; j < n_occ; ++j)
            if (occ[j] == h.tri[k]) at = k;
    }
    bool changed = false;
    const bool walked = at < 0;
    if (at >= 0) changed = hint_hit(h, at);
    else if (walk >= 0) changed = hint_insert(h, walk);
    for (int k = 0; k < N; ++k) rec[k] = h.tri[k];
    return n_tests | ((at + 1) << 8) | ((changed ? 1 : 0) << 16) | ((walked ? 1 : 0) << 17);
}
extern "C" int hint_event(int n, int* rec, int n_tris, const int* occ, int n_occ, int walk, int* tested)
{
    if (n == 1) return event<1>(rec, n_tris, occ, n_occ, walk, tested);
    if (n == 2) return event<2>(rec, n_tris, occ, n_occ, walk, tested);
    if (n == 4) return event<4>(rec, n_tris, occ, n_occ, walk, tested);
    return -1;
}
/* hint_insert alone: what a lane does with an occluder the walk named, whatever the record holds by then */
extern "C" int hint_insert_only(int n, int* rec, int tri)
{
    if (n != 4) return -1;
    OccluderHints<4> h;
    for (int k = 0; k < 4; ++k) h.tri[k] = rec[k];
    const bool changed = hint_insert(h, tri);
    for (int k = 0; k < 4; ++k) rec[k] = h.tri[k];
    return changed ? 1 : 0;
}
extern "C" int hint_empty_record(int* rec)
{
    const OccluderHints<4> h = hint_empty<4>();
    for (int k = 0; k < 4; ++k) rec[k] = h.tri[k];
    return OCCLUDER_HINTS;
}
/* a sequence of events on one record: occ is n_events x max_occ (-1 padded); out: the record after every event, and its return value */
extern "C" void hint_run(int n, int n_tris, int n_events, const int* occ, int max_occ, const int* walk, int* rec, int* recs_out, int* ret_out)
{
    int tested[4];
    for (int e = 0; e < n_events; ++e)
    {
        int cnt = 0;
        while (cnt < max_occ && occ[e * max_occ + cnt] >= 0) ++cnt;
        ret_out[e] = hint_event(n, rec, n_tris, occ + e * max_occ, cnt, walk[e], tested);
        for (int k = 0; k < n; ++k) recs_out[e * n + k] = rec[k];
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="occluder_hint_")
        src, so = os.path.join(d, "hint.cpp"), os.path.join(d, "hint.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC,
                        "-o", so, src], check=True, capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.hint_event.argtypes, L.hint_event.restype = [ci, vp, ci, vp, ci, ci, vp], ci
        L.hint_insert_only.argtypes, L.hint_insert_only.restype = [ci, vp, ci], ci
        L.hint_empty_record.argtypes, L.hint_empty_record.restype = [vp], ci
        L.hint_run.argtypes, L.hint_run.restype = [ci, ci, ci, vp, ci, vp, vp, vp, vp], None
        _lib = L
    return _lib


def event(rec, occ, walk, n_tris=1000):
    """-> (record after, triangles tested, settled position or -1, changed, the walk ran)"""
    r = np.asarray(rec, np.int32).copy()
    o = np.asarray(list(occ) or [0], np.int32)
    tested = np.full(4, -7, np.int32)
    ret = lib().hint_event(len(r), r.ctypes.data, n_tris, o.ctypes.data, len(occ), walk, tested.ctypes.data)
    assert ret >= 0
    return r.tolist(), tested[:ret & 0xff].tolist(), ((ret >> 8) & 0xff) - 1, bool(ret & 0x10000), bool(ret & 0x20000)


def model_event(rec, n, n_tris, occ, walk):
    """most recently used first, no duplicates, n entries, -1 = empty. Returns (tests, settled position, changed)."""
    tests = 0
    for k, t in enumerate(rec):
        if not 0 <= t < n_tris:
            continue
        tests += 1
        if t in occ:
            if k > 0:
                rec.insert(0, rec.pop(k))
            return tests, k, k > 0
    if walk >= 0 and rec[0] != walk:
        if walk in rec:
            rec.remove(walk)
        rec.insert(0, walk)
        del rec[n:]
        return tests, -1, True
    return tests, -1, False


def test_the_source_keeps_one_record_size():
    rec = np.zeros(4, np.int32)
    n = lib().hint_empty_record(rec.ctypes.data)
    assert n in (1, 2, 4) and rec.tolist() == [-1] * 4


def test_an_empty_record_tests_nothing_and_takes_the_walks_occluder():
    for n in (1, 2, 4):
        rec, tested, at, changed, walked = event([-1] * n, [5, 6], 6)
        assert tested == [] and at == -1 and walked and changed and rec == [6] + [-1] * (n - 1)
        rec, tested, at, changed, walked = event([-1] * n, [], -1)  # a visible ray
        assert tested == [] and walked and not changed and rec == [-1] * n


@pytest.mark.parametrize("k", range(4))
def test_a_hit_at_position_k_moves_it_to_the_front(k):
    start = [10, 11, 12, 13]
    rec, tested, at, changed, walked = event(start, [start[k], 99], 99)
    assert tested == start[:k + 1] and at == k and not walked
    assert rec == [start[k]] + start[:k] + start[k + 1:]
    assert changed == (k > 0)  # a hit of the first entry writes nothing
    if k < 2:
        rec2 = event(start[:2], [start[k]], -1)[0]
        assert rec2 == [start[k]] + [t for t in start[:2] if t != start[k]]


def test_insertion_into_a_full_record_drops_the_last_entry():
    rec, tested, at, changed, walked = event([10, 11, 12, 13], [42], 42)
    assert tested == [10, 11, 12, 13] and at == -1 and walked and changed and rec == [42, 10, 11, 12]
    assert event([10, 11], [42], 42)[0] == [42, 10]
    assert event([10], [42], 42)[0] == [42]
    rec, tested, at, changed, walked = event([10, 11, 12, 13], [], -1)  # visible: four tests, the walk, no write
    assert len(tested) == 4 and walked and not changed and rec == [10, 11, 12, 13]


def test_reinserting_a_present_triangle_leaves_no_duplicate():
    """the record is reloaded after the walk: by then it may hold the walk's occluder already (another launch wrote it)"""
    L = lib()
    for start, tri, want, changed in (([10, 11, 12, 13], 12, [12, 10, 11, 13], 1), ([10, 11, 12, 13], 13, [13, 10, 11, 12], 1),
                                      ([10, 11, 12, 13], 10, [10, 11, 12, 13], 0), ([10, 11, -1, -1], 11, [11, 10, -1, -1], 1),
                                      ([10, 11, -1, -1], 12, [12, 10, 11, -1], 1), ([10, 11, 12, 13], -1, [10, 11, 12, 13], 0)):
        r = np.asarray(start, np.int32)
        assert L.hint_insert_only(4, r.ctypes.data, tri) == changed
        assert r.tolist() == want
        live = [t for t in r.tolist() if t >= 0]
        assert len(live) == len(set(live)) and len(live) == min(4, len([t for t in start if t >= 0]) + (tri >= 0 and tri not in start))


def test_entries_that_name_no_triangle_are_never_tested():
    # -1 in front of, between and behind live entries; an index at and above the triangle count (a record older than rt_scene_set)
    rec, tested, at, changed, walked = event([-1, 7, -1, 9], [9], 9, n_tris=10)
    assert tested == [7, 9] and at == 3 and not walked and rec == [9, -1, 7, -1]
    rec, tested, at, changed, walked = event([10, 5000, -1, 3], [], -1, n_tris=10)
    assert tested == [3] and walked and not changed
    rec, tested, at, changed, walked = event([-1, -1, -1, -1], [0], 0, n_tris=10)
    assert tested == [] and rec == [0, -1, -1, -1]
    rec, tested, at, changed, walked = event([-2147483648, 2147483647, -1, 9], [9], 9, n_tris=10)
    assert tested == [9] and at == 3


@pytest.mark.parametrize("n", (1, 2, 4))
def test_ten_thousand_random_events_equal_the_model(n):
    rng = np.random.default_rng(1900 + n)
    n_events, n_tris, max_occ = 10000, 12, 3
    occ = np.full((n_events, max_occ), -1, np.int32)
    walk = np.full(n_events, -1, np.int32)
    for e in range(n_events):
        cnt = int(rng.integers(0, max_occ + 1)) if rng.random() < 0.85 else 0  # 15 % visible rays
        s = rng.choice(n_tris, size=cnt, replace=False)
        occ[e, :cnt] = s
        if cnt:
            walk[e] = s[int(rng.integers(cnt))]  # the any-hit walk names any one of the occluders
    rec = np.full(n, -1, np.int32)
    recs = np.zeros((n_events, n), np.int32)
    ret = np.zeros(n_events, np.int32)
    lib().hint_run(n, n_tris, n_events, occ.ctypes.data, max_occ, walk.ctypes.data, rec.ctypes.data, recs.ctypes.data, ret.ctypes.data)
    m = [-1] * n
    settled = 0
    for e in range(n_events):
        tests, at, changed = model_event(m, n, n_tris, set(occ[e][occ[e] >= 0].tolist()), int(walk[e]))
        assert recs[e].tolist() == m, (e, recs[e].tolist(), m)
        assert (ret[e] & 0xff, ((ret[e] >> 8) & 0xff) - 1, bool(ret[e] & 0x10000)) == (tests, at, changed), e
        live = [t for t in m if t >= 0]
        assert len(live) == len(set(live))
        settled += at >= 0
    assert settled > 1000  # the events reach the hit path
