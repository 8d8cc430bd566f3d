/* Host check of the interval guard of csrc/neighbour_pick.h (tests/test_neighbour_pick_cpu.py compiles and runs it, once plain and once
 * under -fsanitize=address,undefined).
 *
 * Claim under test: for the exact sx = scale * gx, sy = scale * gy of a pick and ANY sx', sy' with |sx' - sx| <= E, |sy' - sy| <= E,
 * a guard that passes returns the integers of neighbour_pick_exact. The fast path does not exist on the host, so sx', sy' are the
 * exact values moved by adversarial offsets: 0, the end points +-E, +-E (1 - 2^-20), and the offsets that put (float)x + sx' on
 * the nearest integer and one unit in the last place of sx' to either side of it (clamped into [-E, +E]).
 *
 * A control guard that is told E / 8 runs beside it and must be caught returning wrong integers.
 *
 *   neighbour_pick_guard_check [cases per radius] -> one line "ok ..." and exit 0, or the first counter-examples and exit 1 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "neighbour_pick.h"

using namespace rt;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

/* the exact pick's floats: the expressions of neighbour_pick_exact up to the conversion */
static void exact_offsets(float rv0, float rv1, float scale, float* sx, float* sy)
{
    const float radius = sqrt_guarded(fmax_dev(-2.0f * pm_logf(rv0), 0.0f));
    const float phi = 2.0f * kPI * rv1;
    float sn_phi, cs_phi;
    pm_sincosf(phi, &sn_phi, &cs_phi);
    const float gx = radius * cs_phi, gy = radius * sn_phi;
    *sx = scale * gx;
    *sy = scale * gy;
}

/* s + d as a binary32 number that is still within E of s (a rounding that left the interval is stepped back towards s) */
static float moved(float s, double d, float E)
{
    float p = (float)((double)s + d);
    for (int i = 0; i < 4 && fabs((double)p - (double)s) > (double)E; ++i) p = nextafterf(p, s);
    return p;
}

/* the offsets for one coordinate; returns how many */
static int offsets(float s, int c, float E, float* out)
{
    int n = 0;
    const double e = (double)E, e1 = e * (1.0 - 1.0 / 1048576.0);
    out[n++] = s;
    out[n++] = moved(s, -e, E);
    out[n++] = moved(s, e, E);
    out[n++] = moved(s, -e1, E);
    out[n++] = moved(s, e1, E);
    /* the nearest integer to the exact sum, reached as nearly as [-E, +E] allows, and its two binary32 neighbours */
    const double sum = (double)c + (double)s;
    double d = nearbyint(sum) - sum;
    if (d > e) d = e;
    if (d < -e) d = -e;
    const float on = moved(s, d, E);
    out[n++] = on;
    const float dn = nextafterf(on, -INFINITY), up = nextafterf(on, INFINITY);
    if (fabs((double)dn - (double)s) <= e) out[n++] = dn;
    if (fabs((double)up - (double)s) <= e) out[n++] = up;
    return n;
}

int main(int argc, char** argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 400000;
    const float radii[3] = {1.0f, 30.0f, 86.0f};
    long bad = 0, control = 0, guarded = 0, passed = 0, plain = 0, plain_passed[3] = {0, 0, 0};
    for (int ri = 0; ri < 3; ++ri)
    {
        const float scale = radii[ri] / 1.96f, E = neighbour_pick_bound(scale);
        if (!(E > 0.0f && E < 0.01f * radii[ri])) { printf("bound %g for radius %g\n", (double)E, (double)radii[ri]); return 1; }
        for (long i = 0; i < cases; ++i)
        {
            const float rv0 = (float)(1u + rnd() % 8388607u) * 1.1920928955078125e-07f, rv1 = (float)(rnd() % 8388608u) * 1.1920928955078125e-07f;
            const uint32_t pick = rnd();
            /* the corners of a 3840 x 2160 frame one time in eight, anywhere in it otherwise */
            const int x = (pick & 7u) == 0 ? ((pick & 8u) ? 3839 : 0) : (int)(rnd() % 3840u);
            const int yi = (pick & 0x70u) == 0 ? ((pick & 0x80u) ? 2159 : 0) : (int)(rnd() % 2160u);
            float sx, sy;
            exact_offsets(rv0, rv1, scale, &sx, &sy);
            int ex, ey;
            neighbour_pick_exact(rv0, rv1, x, yi, scale, &ex, &ey);
            if (ex != f2i_sat((float)x + sx) || ey != f2i_sat((float)yi + sy)) { printf("the check's own exact floats are not the pick's\n"); return 1; }
            float ox[8], oy[8];
            const int nx_off = offsets(sx, x, E, ox), ny_off = offsets(sy, yi, E, oy);
            /* every x offset with the exact y, every y offset with the exact x, and the two moved together */
            for (int a = 0; a < nx_off + ny_off + (nx_off < ny_off ? nx_off : ny_off); ++a)
            {
                float px = sx, py = sy;
                if (a < nx_off) px = ox[a];
                else if (a < nx_off + ny_off) py = oy[a - nx_off];
                else { px = ox[a - nx_off - ny_off]; py = oy[a - nx_off - ny_off]; }
                int gx = 0, gy = 0;
                const bool ok = neighbour_pick_guard(px, py, E, x, yi, &gx, &gy);
                ++guarded;
                if (a == 0) { ++plain; if (ok) ++plain_passed[ri]; }
                /* control: a guard told an eighth of the bound must be caught out by these offsets, or they test nothing */
                int cx = 0, cy = 0;
                if (neighbour_pick_guard(px, py, 0.125f * E, x, yi, &cx, &cy) && (cx != ex || cy != ey)) ++control;
                if (!ok) continue;
                ++passed;
                if (gx != ex || gy != ey)
                {
                    if (bad++ < 10)
                        printf("MISMATCH radius %g rv0 %a rv1 %a x %d yi %d: exact (%d, %d) from (%a, %a), guard passed (%d, %d) from (%a, %a), E %a\n",
                               (double)radii[ri], (double)rv0, (double)rv1, x, yi, ex, ey, (double)sx, (double)sy, gx, gy, (double)px, (double)py, (double)E);
                }
            }
        }
    }
    /* what must fail: rv0 = 0 (the exact offsets are then inf or NaN) and anything not finite */
    {
        const float scale = 30.0f / 1.96f, E = neighbour_pick_bound(scale), inf = INFINITY, nan = NAN;
        int gx, gy;
        float sx, sy;
        const float rv1s[4] = {0.0f, 0.25f, 0.3f, 0.75f};
        for (int j = 0; j < 4; ++j)
        {
            exact_offsets(0.0f, rv1s[j], scale, &sx, &sy);
            if (neighbour_pick_guard(sx, sy, E, 100, 100, &gx, &gy)) { printf("guard passed for rv0 = 0, rv1 = %g\n", (double)rv1s[j]); ++bad; }
        }
        const float nf[3] = {inf, -inf, nan};
        for (int j = 0; j < 3; ++j)
        {
            if (neighbour_pick_guard(nf[j], 1.5f, E, 100, 100, &gx, &gy)) { printf("guard passed for sx = %g\n", (double)nf[j]); ++bad; }
            if (neighbour_pick_guard(1.5f, nf[j], E, 100, 100, &gx, &gy)) { printf("guard passed for sy = %g\n", (double)nf[j]); ++bad; }
            if (neighbour_pick_guard(nf[j], nf[(j + 1) % 3], E, 0, 0, &gx, &gy)) { printf("guard passed for two non-finite offsets\n"); ++bad; }
            if (neighbour_pick_guard(1.5f, 1.5f, nf[j], 100, 100, &gx, &gy)) { printf("guard passed for E = %g\n", (double)nf[j]); ++bad; }
        }
        /* and a plain value in the middle of a pixel passes */
        if (!neighbour_pick_guard(1.5f, -2.5f, E, 100, 100, &gx, &gy) || gx != 101 || gy != 97) { printf("guard failed in the middle of a pixel\n"); ++bad; }
    }
    if (cases >= 100000 && control == 0) { printf("the offsets never caught a guard with an eighth of the bound\n"); ++bad; }
    if (bad) { printf("FAILED: %ld\n", bad); return 1; }
    printf("ok control_caught %ld cases_per_radius %ld guard_calls %ld passed %ld unmoved %ld unmoved_passed_r1 %ld unmoved_passed_r30 %ld unmoved_passed_r86 %ld\n",
           control, cases, guarded, passed, plain, plain_passed[0], plain_passed[1], plain_passed[2]);
    return 0;
}
