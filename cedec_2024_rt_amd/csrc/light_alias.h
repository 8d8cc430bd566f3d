/*
 * light_alias.h — power-proportional light selection for the ReSTIR candidates (rt_light_sampling): the alias
 * table, its host builder and the one selection function the kernel (frame_kernels.h, k_generate_candidate<.., POWER>) and the CPU
 * restatement (tests/light_sampling_ref.py) share. Plain C++; RT_HD where the device needs it.
 *
 * Light i (the light list's index order) has the weight w_i = tri_area(v0, v1, v2) * luminance(Ke), binary32, the functions of
 * rt_device.h. The weights are quantised to integers q_i relative to the largest finite one,
 *     q_i = max(1, floor(w_i / w_max * 2^32 + 1/2))   for 0 < w_i < inf,        q_i = 0 otherwise (zero area, NaN, inf),
 * T = sum q_i. Everything after that is exact integer arithmetic: q_i <= 2^32 and L <= 2^26, so the masses m_i = q_i L and the slot
 * capacity T stay below 2^58; only the last step, m 2^23 / T, needs 128 bits.
 *
 * Table (Vose 1991). Slot s holds {thr_s, alias_s}. Lights with m_i < T are "small", the others "large"; both lists are stacks
 * filled in index order. While both hold an entry: pop small s and large l; slot s keeps m_s of its own light and gives the rest of
 * its capacity, T - m_s, to l; m_l -= T - m_s, and l goes back onto the list its new mass says. The sum of the masses still on a list
 * is always T times their number, so the lists run out together except for large entries with m = T exactly: those slots are full
 * (thr = 2^23, alias = the slot itself). Then, and only then, something rounds:
 *     thr_s = floor(m_s 2^23 / T + 1/2), raised to 1 if q_s > 0,      0 <= thr_s <= 2^23
 * (PCG::uniformf delivers 23 bits: a finer threshold could not be told apart). A light with q = 0 gets thr = 0 and is no alias (an
 * alias was large: m >= T > 0), so it is never selected; a light with q > 0 keeps at least one of the 2^23 values of its own slot.
 *
 * Realised count. Given a uniform slot and a uniform 23-bit integer, light i is selected by K_i of the L 2^23 equally likely pairs,
 *     K_i = thr_i + sum over s with alias_s = i of (2^23 - thr_s)            (a full slot's own term is 0),      sum K_i = L 2^23.
 * The pdf the kernel divides by is K_i / (L 2^23) * 1 / area: the probability the table REALISES, not w_i / sum w. The estimator is
 * unbiased for any pdf that is positive where the integrand is and is the one sampled from; the quantisation moves the variance by
 * a hair and the expectation not at all.
 *
 * Error bound. With the exact share E_i = q_i L 2^23 / T = (m_i / T) 2^23: every unit of m_i is kept by the own slot or given to
 * light i by a slot that names it as alias, in exact arithmetic. A slot's threshold differs from its exact value m_s 2^23 / T by at
 * most 1/2 from the rounding, or by less than 1 where the floor of 1 applies (exact value in (0, 1/2)); that error enters the
 * count of the slot's own light and, with the other sign, of its alias. So
 *     |K_i - E_i| <= (number of slots that name i: its own, and those with alias_s = i),
 * checked on the CPU by tests/test_light_sampling_cpu.py. The slot itself is drawn as floor(rv0 L) with the clamp, exactly as the
 * reference draws its light (common/core.hpp:261-285): rv0 has 23 bits too, so for L that is no power of two the slots are not
 * exactly equally likely; that granularity is the reference's own (its 1 / L has it) and is kept, see DESIGN.md section 12.
 */
#pragma once
#include <stdint.h>

#include "rt_device.h"

#include <vector>

namespace rt
{

constexpr uint32_t kAliasOne = 1u << 23; /* a threshold that always takes the slot's own light */

struct AliasSlot
{
    uint32_t thr, alias;
};

/* the 23-bit integer PCG::uniformf made ra from: ra = k 2^-23 exactly */
RT_HD uint32_t alias_bits(float ra) { return (uint32_t)(ra * 8388608.0f); }
/* the slot of rv0: the reference's light index (common/core.hpp:261-285), clamp included */
RT_HD uint32_t light_slot(uint32_t L, float rv0)
{
    uint32_t s = (uint32_t)(rv0 * (float)(size_t)L);
    if (s == L) s = L - 1u;
    return s;
}
/* the slot's own light iff ra's integer is below the slot's threshold */
RT_HD uint32_t light_select_slot(AliasSlot e, uint32_t slot, float ra) { return alias_bits(ra) < e.thr ? slot : e.alias; }
RT_HD uint32_t light_select(const AliasSlot* table, uint32_t L, float rv0, float ra)
{
    const uint32_t s = light_slot(L, rv0);
    return light_select_slot(table[s], s, ra);
}
/* weight of a light from its vertices and emission [parity: binary32, this order] */
RT_HD float light_weight(f3 v0, f3 v1, f3 v2, f3 ke) { return tri_area(v0, v1, v2) * luminance(ke); }
/* the probability the table selects light i with, as the binary32 factor of its pdf: pdf = light_select_prob(K, L) * 1.0f / area */
RT_HD float light_select_prob(uint64_t K, uint32_t L) { return (float)((double)K / ((double)L * 8388608.0)); }

/* ---- the host's builder (the device pass of hipcc parses it too and emits nothing) */
inline bool light_weight_ok(float w) { return w > 0.0f && w <= kFltMax; } /* positive and finite; NaN fails both */

/* q per light; returns T */
inline uint64_t alias_quantise(const float* w, uint32_t L, std::vector<uint64_t>& q)
{
    q.assign(L, 0u);
    float w_max = 0.0f;
    for (uint32_t i = 0; i < L; ++i)
        if (light_weight_ok(w[i]) && w[i] > w_max) w_max = w[i];
    uint64_t T = 0u;
    for (uint32_t i = 0; i < L; ++i)
    {
        if (!light_weight_ok(w[i])) continue;
        const uint64_t v = (uint64_t)((double)w[i] / (double)w_max * 4294967296.0 + 0.5); /* <= 2^32; the product is exact in binary64 */
        q[i] = v < 1u ? 1u : v;
        T += q[i];
    }
    return T;
}

/* The table and the realised counts of L weights. false (table and K zeroed) if no light has q > 0. */
inline bool alias_build(const float* w, uint32_t L, std::vector<AliasSlot>& table, std::vector<uint64_t>& K)
{
    std::vector<uint64_t> q;
    const uint64_t T = alias_quantise(w, L, q);
    table.assign(L, AliasSlot{0u, 0u});
    K.assign(L, 0u);
    if (T == 0u) return false;
    std::vector<uint64_t> m(L), keep(L);
    std::vector<uint32_t> small, large;
    for (uint32_t i = 0; i < L; ++i)
    {
        m[i] = q[i] * (uint64_t)L;
        (m[i] < T ? small : large).push_back(i);
    }
    for (uint32_t i = 0; i < L; ++i) { keep[i] = T; table[i].alias = i; } /* full unless paired below */
    while (!small.empty() && !large.empty())
    {
        const uint32_t s = small.back(), l = large.back();
        small.pop_back(); large.pop_back();
        keep[s] = m[s];
        table[s].alias = l;
        m[l] -= T - m[s];
        (m[l] < T ? small : large).push_back(l);
    }
    /* exact arithmetic leaves nothing on `small` (header comment); a slot left there would be full like the rest */
    for (uint32_t s = 0; s < L; ++s)
    {
        uint32_t thr = (uint32_t)((((unsigned __int128)keep[s] << 24) / T + 1u) >> 1); /* floor(keep 2^23 / T + 1/2) */
        if (q[s] > 0u && thr < 1u) thr = 1u;
        table[s].thr = thr;
    }
    for (uint32_t s = 0; s < L; ++s)
    {
        K[s] += table[s].thr;
        K[table[s].alias] += kAliasOne - table[s].thr;
    }
    return true;
}

}  // namespace rt
