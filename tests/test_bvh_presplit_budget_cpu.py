"""The pre-split's fragment length stays within its budget (csrc/bvh_fragment.h::frag_fit_length, the one search both builders
call), on the CPU: the header compiled by the g++ line of tests/test_bvh_fragment_cpu.py, counting with the header's own
frag_split.

"Before" is the loop both builders had (restated below as fit_old): 16 counts, 1.5 x between them, then on with whatever the
count is. On a tessellated object among large walls (bvh_build_scenes.budget_scene) it ends far over 4 * triangles + 1024; the
new search must end within it for every input, and must not move a scene whose first lengths fitted.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bvh_build_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedec_2024_rt_amd", "csrc")

PROGRAM = r"""
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "bvh_fragment.h"

#include <map>
#include <thread>
#include <vector>

/* total fragments of the scene at length L by the header's frag_split, over a few threads (a count of the larger scenes is
 * 30 M fragments); one scene's counts are kept per length, so that "before", "after" and the checks share them */
static int g_calls;
static float g_lengths[512];
static const float* g_tris;
static int g_n;
static std::map<uint32_t, uint64_t> g_memo;
extern "C" uint64_t count_at(const float* tris /* 9 floats each */, int n, float L)
{
    if (g_calls < 512) g_lengths[g_calls] = L;
    ++g_calls;
    if (tris != g_tris || n != g_n) { g_memo.clear(); g_tris = tris; g_n = n; }
    uint32_t key;
    memcpy(&key, &L, 4);
    auto hit = g_memo.find(key);
    if (hit != g_memo.end()) return hit->second;
    const int nt = n < 256 ? 1 : 8;
    std::vector<uint64_t> part((size_t)nt, 0);
    std::vector<std::thread> th;
    auto work = [&](int k) {
        uint64_t total = 0;
        for (int i = k; i < n; i += nt)
            total += rt::frag_split<false>(tris + 9 * (size_t)i, L, [](uint32_t, const rt::FragPoly<false>&, const float*, const float*) {});
        part[(size_t)k] = total;
    };
    for (int k = 1; k < nt; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& t : th) t.join();
    uint64_t total = 0;
    for (uint64_t v : part) total += v;
    g_memo[key] = total;
    return total;
}
/* the header's search; calls = how many lengths it counted, lengths = which */
extern "C" float fit_new(const float* tris, int n, float L0, uint64_t budget, uint64_t* total, int* calls, float* lengths)
{
    g_calls = 0;
    const float L = rt::frag_fit_length(L0, budget, [&](float len) { return count_at(tris, n, len); }, total);
    *calls = g_calls;
    for (int i = 0; i < g_calls && i < 512; ++i) lengths[i] = g_lengths[i];
    return L;
}
/* ---- the loop of build_bvh_device and of the host path as it was, restated ---- */
extern "C" float fit_old(const float* tris, int n_tris, float L, uint64_t* total)
{
    const size_t budget = (size_t)n_tris * 4 + 1024;
    uint64_t n = 0;
    for (int it = 0; it < 16; ++it)
    {
        n = count_at(tris, n_tris, L);
        if ((size_t)n <= budget || L <= 0.0f) break;
        L *= 1.5f;
    }
    *total = n;
    return L;
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="frag_fit_")
        src, so = os.path.join(d, "frag_fit.cpp"), os.path.join(d, "frag_fit.so")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-I", CSRC, "-o", so, src], check=True,
                       capture_output=True, timeout=300)
        L = C.CDLL(so)
        vp, f32, u64 = C.c_void_p, C.c_float, C.c_uint64
        L.count_at.argtypes, L.count_at.restype = [vp, C.c_int, f32], u64
        L.fit_new.argtypes, L.fit_new.restype = [vp, C.c_int, f32, u64, vp, vp, vp], f32
        L.fit_old.argtypes, L.fit_old.restype = [vp, C.c_int, f32, vp], f32
        _lib = L
    return _lib


_FLAT = {}


def _flat(v):
    """(n, 9) float32 of v, one array per scene and kept: the program above keeps a scene's counts by the array's address"""
    if id(v) not in _FLAT:
        _FLAT[id(v)] = (v, np.array(v, np.float32).reshape(-1, 9))
    return _FLAT[id(v)][1]


def budget_of(n_tris):
    return 4 * n_tris + 1024


def fit_new(v, L0, budget=None):
    t = _flat(v)
    total, calls, lengths = C.c_uint64(), C.c_int(), np.zeros(512, np.float32)
    L = lib().fit_new(t.ctypes.data, len(t), np.float32(L0), budget_of(len(t)) if budget is None else budget, C.byref(total), C.byref(calls),
                      lengths.ctypes.data)
    return np.float32(L), total.value, lengths[:calls.value]


def fit_old(v, L0):
    t = _flat(v)
    total = C.c_uint64()
    L = lib().fit_old(t.ctypes.data, len(t), np.float32(L0), C.byref(total))
    return np.float32(L), total.value


def count_at(v, L):
    t = _flat(v)
    return lib().count_at(t.ctypes.data, len(t), np.float32(L))


FINDING_4 = [(2000, 0.1), (20000, 0.1), (2000, 0.4), (20000, 0.4)]


@pytest.mark.parametrize("n,large", FINDING_4)
def test_walls_and_tessellation_fit_the_budget(n, large):
    """the loop as it was ends after 16 rounds far over the budget; frag_fit_length ends within it, by the same 16 lengths
    followed by doublings, and the count it reports is the count at the length it returns"""
    v = S.budget_scene(n, large)
    L0 = S.split_length(v, 10.0)
    budget = budget_of(n)
    old_L, old_n = fit_old(v, L0)
    print(f"{n} triangles, {large:.0%} large: before {old_n} references at L = {old_L} (budget {budget})")
    assert old_n > budget, "the input does not show the defect it is here for"
    L, total, lengths = fit_new(v, L0)
    print(f"  after {total} references at L = {L}, {len(lengths)} counts")
    assert total <= budget
    assert total >= n
    assert L == lengths[-1] and count_at(v, L) == total
    # the first 16 lengths are the old loop's, in binary32; after them L doubles
    want = [np.float32(L0)]
    for _ in range(15):
        want.append(np.float32(want[-1] * np.float32(1.5)))
    assert len(lengths) > 16 and [x.tobytes() for x in lengths[:16]] == [x.tobytes() for x in want]
    assert all(lengths[i + 1] == np.float32(2.0) * lengths[i] for i in range(15, len(lengths) - 1))
    # and it is the first of them that fits
    assert count_at(v, lengths[-2]) > budget


def test_a_scene_that_fits_keeps_its_first_length():
    """all triangles of one size: ten median extents cut nothing, one count"""
    v = S.equal_size_scene()
    L0 = S.split_length(v, 10.0)
    L, total, lengths = fit_new(v, L0)
    assert L.tobytes() == np.float32(L0).tobytes() and len(lengths) == 1 and total == len(v) <= budget_of(len(v))
    assert fit_old(v, L0) == (L, total)


def test_lengths_reached_by_the_old_steps_are_kept_bit_for_bit():
    """where the 1.5 x steps converge, the search returns what the loop as it was returned: a budget scene scaled so that a few
    steps are enough, and a split factor small enough to cut an equal-size scene"""
    cases = [(S.equal_size_scene(), 0.05), (S.equal_size_scene(300, 3), 0.02)]
    v = S.budget_scene(2000, 0.1).copy()
    cases.append((v, 10.0 * 2000.0))  # L0 = 2e4 medians = a few units: the walls are cut a few times each
    steps = []
    for v, factor in cases:
        L0 = S.split_length(v, factor)
        old_L, old_n = fit_old(v, L0)
        assert old_n <= budget_of(len(v)), "the old loop converges on this input"
        L, total, lengths = fit_new(v, L0)
        assert (L.tobytes(), total) == (old_L.tobytes(), old_n)
        steps.append(len(lengths))
    assert max(steps) > 1, f"no case needed a step: {steps}"


def test_one_triangle_longer_than_its_length():
    """one triangle of extent 8 with L0 = 0.001: capped at FRAG_MAX_PER_TRI fragments against a budget of 1028, so L grows; and
    with a budget below what the 16 steps reach, the doublings end it"""
    v = np.asarray([[[0, 0, 0], [8, 0, 0], [0, 8, 1]]], np.float32)
    assert count_at(v, 0.001) > budget_of(1)
    L, total, lengths = fit_new(v, 0.001)
    assert 1 <= total <= budget_of(1) and len(lengths) > 1 and count_at(v, L) == total
    L, total, lengths = fit_new(v, 0.001, budget=1)
    assert total == 1 and L >= 8.0 and len(lengths) > 16


def test_no_length_means_no_search():
    """split factor 0 (L = 0): one reference per triangle, one count, also against a budget it cannot meet"""
    v = S.equal_size_scene(50)
    for budget in (None, 3):
        L, total, lengths = fit_new(v, 0.0, budget=budget)
        assert L == 0.0 and total == len(v) and len(lengths) == 1
